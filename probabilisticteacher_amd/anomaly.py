"""Anomaly mode: find the first non-finite tensor of a train step and stop before the update.

The reference runs every step under `torch.autograd.set_detect_anomaly(True)` (pt/engine/trainer.py:167): a diverging run raises
out of `backward()`, names the backward node and never reaches `optimizer.step()`.  Here `PTrainer(cfg, detect_anomaly=True)`
gives every autograd function of `ops.py` / `p8.py` an `AnomalySink`: each tensor a function returns from `forward` and each
gradient it returns from `backward` is scanned by one launch of `ptmi_nonfinite_scan` (csrc/anomaly.hip) into the sink's next
slot -- two flag bits and the lowest non-finite index, on the device.  After `backward()` one `ptmi_seg_nonfinite` launch flags
the parameters whose gradient is non-finite, `collect()` reads the flags back in ONE copy, and the trainer raises `AnomalyError`
BEFORE the fused clip + SGD step: parameters, momentum and iteration stay what they were.

Everything here is host bookkeeping; the two kernels are the only device work and there is no CPU path (the CPU tests drive a
sink whose `_launch` / `_fetch` are replaced)."""
from __future__ import annotations

import ctypes
import json
from dataclasses import asdict, dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

INT64_MAX = 2 ** 63 - 1
KINDS = {1: "nan", 2: "inf", 3: "nan+inf"}
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


def p8_decode(offset: int, n: int, c: int, h: int, w: int):
    """Flat element offset in the P8 layout t[2 ceil(C/16)][N (H + 1) + 1][W + 1][8] (include/ptmi355.h) -> (image, channel, y,
    x), or "halo" for the zero rows between the images / column 0 (the convolution's padding), or "channel padding" for a channel
    >= C of the last 16-channel chunk.  Pure host arithmetic."""
    planes, rows, ws = 2 * (-(-c // 16)), n * (h + 1) + 1, w + 1
    if not 0 <= offset < planes * rows * ws * 8:
        raise ValueError(f"offset {offset} outside a P8 tensor of {planes} x {rows} x {ws} x 8 elements")
    lane = offset % 8
    col = (offset // 8) % ws
    row = (offset // (8 * ws)) % rows
    plane = offset // (8 * ws * rows)
    if col == 0 or row % (h + 1) == 0:
        return "halo"
    ch = plane * 8 + lane
    if ch >= c:
        return "channel padding"
    return ((row - 1) // (h + 1), ch, (row - 1) % (h + 1), col - 1)


def unravel(offset: int, shape: Sequence[int]) -> Tuple[int, ...]:
    """coordinate of a flat offset in a contiguous tensor of `shape` (row-major); () for a scalar"""
    out = []
    for d in reversed(tuple(shape)):
        out.append(offset % d)
        offset //= d
    return tuple(reversed(out))


@dataclass
class AnomalyRecord:
    """one scanned tensor that held a NaN or an infinity"""
    phase: str                  # "forward" | "backward"
    branch: str                 # "supervised" | "unsupervised" | "unsup_data_weak" | "joint" | ""
    scope: str                  # state-dict-like path of the module, e.g. "roi_heads.box_predictor.cls_score"
    op: str                     # the autograd function
    output: str                 # which of its results
    kind: str                   # "nan" | "inf" | "nan+inf"
    shape: tuple
    dtype: str
    first_index: int            # lowest flat index of a non-finite element
    coordinate: object          # its coordinate: a tuple, or "halo" / "channel padding" inside a P8 tensor

    def describe(self) -> str:
        return (f"{self.phase} of {self.branch or '-'} / {self.scope or '-'}: {self.op} -> {self.output} "
                f"({self.dtype} {list(self.shape)}) holds {self.kind}, first at flat index {self.first_index} = {self.coordinate}")

    def to_dict(self) -> dict:
        d = asdict(self)
        d["shape"] = list(self.shape)
        d["coordinate"] = list(self.coordinate) if isinstance(self.coordinate, tuple) else self.coordinate
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "AnomalyRecord":
        d = dict(d)
        d["shape"] = tuple(d["shape"])
        if isinstance(d["coordinate"], list):
            d["coordinate"] = tuple(d["coordinate"])
        return cls(**d)


class AnomalyError(FloatingPointError):
    """Raised by PTrainer(detect_anomaly=True) BEFORE the update of a step that produced a non-finite tensor or gradient.
    iteration: the step;  records: AnomalyRecords in execution order (this rank's);  parameters: [(name, kind)] of the trainable
    parameters whose gradient segment is non-finite, in named_parameters() order;  reporting_ranks: the ranks that had records
    (multi-rank runs: every rank raises in the same step, also one that saw nothing itself)."""

    def __init__(self, iteration: int, records: Sequence[AnomalyRecord] = (), parameters: Sequence[Tuple[str, str]] = (),
                 reporting_ranks: Sequence[int] = (), note: str = ""):
        self.iteration = int(iteration)
        self.records = list(records)
        self.parameters = [(str(n), str(k)) for n, k in parameters]
        self.reporting_ranks = [int(r) for r in reporting_ranks]
        self.note = str(note)
        super().__init__(self._message())

    @property
    def parameter_names(self) -> List[str]:
        return [n for n, _ in self.parameters]

    def _message(self) -> str:
        head = f"non-finite values at iteration {self.iteration}, the update was not applied"
        if self.records:
            lines = [f"{head}; first: {self.records[0].describe()}"]
            if len(self.records) > 1:
                lines.append(f"{len(self.records)} records in execution order; the next ones:")
                lines += ["  " + r.describe() for r in self.records[1:6]]
        else:
            lines = [f"{head}; no tensor scanned on this rank was non-finite"]
        if self.reporting_ranks:
            lines.append("ranks that reported records: " + ", ".join(str(r) for r in self.reporting_ranks))
        if self.parameters:
            shown = ", ".join(f"{n} ({k})" for n, k in self.parameters[:8])
            more = f" and {len(self.parameters) - 8} more" if len(self.parameters) > 8 else ""
            lines.append(f"non-finite gradient in {len(self.parameters)} parameter(s): {shown}{more}")
        if self.note:
            lines.append(self.note)
        return "\n".join(lines)

    def __reduce__(self):       # (crosses multiprocessing queues: rebuild from the fields, not from the message)
        return (AnomalyError, (self.iteration, self.records, self.parameters, self.reporting_ranks, self.note))

    def to_dict(self) -> dict:
        return {"iteration": self.iteration, "records": [r.to_dict() for r in self.records],
                "parameters": [{"name": n, "kind": k} for n, k in self.parameters], "reporting_ranks": self.reporting_ranks,
                "note": self.note, "message": str(self)}

    def to_json(self) -> str:
        return json.dumps(self.to_dict(), indent=1, sort_keys=True)

    @classmethod
    def from_json(cls, text: str) -> "AnomalyError":
        d = json.loads(text)
        return cls(d["iteration"], [AnomalyRecord.from_dict(r) for r in d["records"]],
                   [(p["name"], p["kind"]) for p in d["parameters"]], d.get("reporting_ranks", ()), d.get("note", ""))


class AnomalySink:
    """Device flags + first indices of the tensors scanned in one step, and the host list of what each slot is.

    One int32 array [segments | capacity] and one int64 array [capacity]: `seg_flags` (the first `segments` words) is where
    `ops.seg_nonfinite` writes the per-parameter gradient flags, so that `collect()` reads them and the slots' flags back in ONE
    device->host copy; the first indices follow in a second copy only if some flag is set."""

    def __init__(self, device, capacity: int = 4096, segments: int = 0):
        if capacity < 1 or segments < 0:
            raise ValueError("an anomaly sink needs a positive capacity")
        self.device, self.capacity, self.segments = device, int(capacity), int(segments)
        self._slots: List[tuple] = []
        self.segment_flags: List[int] = [0] * self.segments       # host copy, as of the last collect()
        self.last_used = 0                                        # slots the last collected step took
        self._alloc()

    # ---- device side (replaced by the CPU tests' fake)
    def _alloc(self) -> None:
        self.flags = torch.zeros(self.segments + self.capacity, dtype=torch.int32, device=self.device)
        self.first = torch.full((self.capacity,), INT64_MAX, dtype=torch.int64, device=self.device)
        self.seg_flags = self.flags[: self.segments]

    def _reset(self) -> None:
        self.flags.zero_()
        self.first.fill_(INT64_MAX)

    def _launch(self, tensor: torch.Tensor, dtype: int, slot: int) -> None:
        stream = ctypes.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)
        _lib.call("ptmi_nonfinite_scan", ctypes.c_void_p(tensor.data_ptr()), tensor.numel(), dtype,
                  ctypes.c_void_p(self.flags.data_ptr() + 4 * self.segments), ctypes.c_void_p(self.first.data_ptr()), slot,
                  self.capacity, stream)

    def _fetch_flags(self, used: int) -> List[int]:
        return self.flags[: self.segments + used].cpu().tolist()

    def _fetch_first(self, used: int) -> List[int]:
        return self.first[:used].cpu().tolist()

    # ---- interface
    @property
    def used(self) -> int:
        return len(self._slots)

    def begin_step(self) -> None:
        self._reset()
        self._slots = []

    def scan(self, tensor: torch.Tensor, phase: str, op: str, output: str, branch: str = "", scope: str = "",
             p8: Optional[Tuple[int, int, int, int]] = None) -> None:
        """take the next slot for `tensor` and launch the scan.  p8 = (n, c, h, w) of a P8 tensor (its whole allocation is
        scanned: every producer defines all of it, pads included).  Tensors of other dtypes than fp32 / bf16 (argmax maps,
        masks) and empty tensors cannot hold a non-finite value and take no slot."""
        code = _DTYPES.get(tensor.dtype)
        if code is None or tensor.numel() == 0:
            return
        if len(self._slots) >= self.capacity:
            raise RuntimeError(f"anomaly sink: this step scans more than {self.capacity} tensors (at {phase} {scope or '-'} {op} -> "
                               f"{output}); construct the AnomalySink with a larger capacity")
        if not tensor.is_contiguous():
            tensor = tensor.contiguous()
        slot = len(self._slots)
        self._slots.append((phase, branch, scope, op, output, tuple(tensor.shape), str(tensor.dtype).replace("torch.", ""), p8))
        self._launch(tensor, code, slot)

    def collect(self) -> List[AnomalyRecord]:
        """records of the slots that hold a flag, in execution order; also refreshes `segment_flags` and `last_used`"""
        used = len(self._slots)
        self.last_used = used
        flags = self._fetch_flags(used)
        self.segment_flags, flags = flags[: self.segments], flags[self.segments:]
        if not any(flags):
            return []
        first = self._fetch_first(used)
        out = []
        for (phase, branch, scope, op, output, shape, dtype, p8), f, i in zip(self._slots, flags, first):
            if not f:
                continue
            coord = p8_decode(i, *p8) if p8 is not None else unravel(i, shape)
            out.append(AnomalyRecord(phase, branch, scope, op, output, KINDS[f & 3], shape, dtype, int(i), coord))
        return out


def flagged_parameters(segment_flags: Sequence[int], segment_names: Sequence[str], order: Sequence[str]) -> List[Tuple[str, str]]:
    """[(name, kind)] of the segments with a flag, listed in `order` (named_parameters() order)"""
    kind = {n: KINDS[f & 3] for n, f in zip(segment_names, segment_flags) if f & 3}
    return [(n, kind[n]) for n in order if n in kind]
