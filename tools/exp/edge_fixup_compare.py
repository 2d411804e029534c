#!/usr/bin/env python
"""Builds of libptmi355.so against each other in ONE process on the F(2x2,3x3)-domain weight gradient (csrc/wino.hip,
ptmi_conv3x3_wino_wgrad): the sibling of handover_compare.py, which does the same for the F(4x4,3x3) kernels and whose
helpers this uses.  The first library is the base of every comparison.

    python tools/exp/edge_fixup_compare.py time-wgrad2 --libs parent.so,new.so [--n 48] [--layers conv5_1,..] [--reps 2]
        as handover_compare.py time-wgrad: every repetition walks the libraries in alternating order; per library and layer the
        ms of each repetition, the mean's ratio to the base, "same bits as base", and the job's largest repeat spread
    python tools/exp/edge_fixup_compare.py bitident --libs parent.so,new.so [--n 48]
        torch.equal of dW / db on the shapes of tests/test_wino_wgrad_setup_gpu.py and on the layer shapes at n images; and of the
        F(4x4,3x3) forward (epilogues 1, 4) and dgrad (2, 3), both tile schedules, on the shapes of tests/test_wino_edge_fixup_gpu.py
        and on five layer shapes at n images (timing of that kernel: handover_compare.py time-fwd)"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handover_compare as hc  # noqa: E402

vp, DEV = hc.vp, hc.DEV
# the maps ops routes to this kernel at 1333x800: conv5_x and the RPN convolution, all 512 -> 512 at 50x83; the others for reference
LAYERS = {"conv5_1": (512, 512, 50, 83), "conv4_2": (512, 512, 100, 166), "conv3_2": (256, 256, 200, 333)}
FWD_BITIDENT = ("conv1_2", "conv3_2", "conv4_1", "conv4_2", "conv5_1")      # the forward / dgrad kernel (csrc/wino4p.hip): bitident only


def load(spec):
    libs = hc.load(spec)
    for _, lib in libs:
        lib.ptmi_conv3x3_wino_wgrad_ws_floats.restype = ctypes.c_int64
    return libs


def wgrad2_call(lib, x, dy, out=None):
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    if out is None:
        out = (torch.full((cout, cin, 3, 3), float("nan"), device=DEV), torch.full((cout,), float("nan"), device=DEV),
               torch.empty(lib.ptmi_conv3x3_wino_wgrad_ws_floats(n, cin, cout, h, w), device=DEV))
    dw, db, ws = out
    assert lib.ptmi_conv3x3_wino_wgrad(vp(x.data_ptr()), vp(dy.data_ptr()), vp(dw.data_ptr()), vp(db.data_ptr()), vp(ws.data_ptr()),
                                       n, cin, cout, h, w, 0, hc.stream()) == 0
    return out


def time_mode(a, libs):
    worst = 0.0
    for name in (a.layers.split(",") if a.layers else ["conv5_1"]):
        cin, cout, h, w = LAYERS[name]
        gen = torch.Generator(device=DEV).manual_seed(1)
        x, dy = torch.relu(hc.rand(gen, a.n, cin, h, w)), hc.rand(gen, a.n, cout, h, w)
        outs = [wgrad2_call(lib, x, dy) for _, lib in libs]
        runs = [lambda lib=lib, o=o: wgrad2_call(lib, x, dy, o) for (_, lib), o in zip(libs, outs)]
        ms = [[] for _ in libs]
        for rep in range(a.reps):
            order = range(len(libs)) if rep % 2 == 0 else reversed(range(len(libs)))
            for i in order:
                ms[i].append(hc.timed(runs[i], a.iters))
        base = sum(ms[0]) / len(ms[0])
        for i, (lname, _) in enumerate(libs):
            mean = sum(ms[i]) / len(ms[i])
            spread = (max(ms[i]) - min(ms[i])) / min(ms[i])
            worst = max(worst, spread)
            same = all(torch.equal(p, q) for p, q in zip(outs[0][:2], outs[i][:2]))
            print(f"{name:8s} n={a.n:2d} {lname:28s} " + " ".join(f"{t:8.4f}" for t in ms[i]) + f" ms  mean {mean:8.4f}  x{mean / base:.4f} of base"
                  f"  ({(mean / base - 1) * 100:+.2f} %)  repeat spread {spread * 100:.2f} %  same bits as base {same}", flush=True)
    print(f"largest repeat spread of one library on one layer in this job: {worst * 100:.2f} %")


def bitident(a, libs):
    sys.path.insert(0, os.path.join(hc.ROOT, "tests"))
    from test_wino_edge_fixup_gpu import SHAPES as FWD_SHAPES
    from test_wino_wgrad_setup_gpu import SHAPES
    (_, old), (_, new) = libs[:2]
    bad = 0
    sched = torch.zeros(16, dtype=torch.int32, device=DEV)
    for (n, cin, cout, h, w), tag in [(s, "test") for s in FWD_SHAPES] + [((a.n,) + hc.FWD_LAYERS[k], k) for k in FWD_BITIDENT]:
        gen = torch.Generator(device=DEV).manual_seed(n + cin + cout + h + w)
        x, gy, mask = torch.relu(hc.rand(gen, n, cin, h, w)), hc.rand(gen, n, cout, h, w), hc.rand(gen, n, cin, h, w)
        wt, b = hc.rand(gen, cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, hc.rand(gen, cout) * 0.1
        res = []
        for sc in (None, sched):
            for epi in (1, 4, 2, 3):
                if epi == 4 and (h % 2 or w % 2):
                    continue
                args = (x, wt, b, None, epi, 0) if epi in (1, 4) else (gy, wt, None, mask if epi == 3 else None, epi, 1)
                yo = hc.fwd_call(old, *args, sched=sc)
                yn = hc.fwd_call(new, *args, sched=sc)
                ok = torch.equal(yo, yn) and bool(torch.isfinite(yn).all())
                bad += not ok
                res.append(f"{'dyn' if sc is not None else 'stat'}/{epi}:{'equal' if ok else 'DIFFER'}")
                del yo, yn
        print(f"fwd/dgrad F(4x4) {tag:8s} n={n} {cin}->{cout} {h}x{w}  " + " ".join(res), flush=True)
        del x, gy, mask
    for (n, cin, cout, h, w), tag in [(s, "test") for s in SHAPES] + [((a.n,) + LAYERS[k], k) for k in LAYERS]:
        gen = torch.Generator(device=DEV).manual_seed(n + cin + cout + h + w)
        x, dy = torch.relu(hc.rand(gen, n, cin, h, w)), hc.rand(gen, n, cout, h, w)
        o, nw = wgrad2_call(old, x, dy), wgrad2_call(new, x, dy)
        ok = torch.equal(o[0], nw[0]) and torch.equal(o[1], nw[1]) and bool(torch.isfinite(nw[0]).all() and torch.isfinite(nw[1]).all())
        bad += not ok
        print(f"wgrad F(2x2) {tag:8s} n={n} {cin}->{cout} {h}x{w}  dW, db {'equal' if ok else 'DIFFER'}", flush=True)
        del o, nw, x, dy
    print("all identical" if not bad else f"{bad} DIFFER")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time-wgrad2", "bitident"])
    ap.add_argument("--libs", required=True)
    ap.add_argument("--n", type=int, default=48)
    ap.add_argument("--layers", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    libs = load(a.libs)
    if a.mode == "bitident":
        return bitident(a, libs)
    time_mode(a, libs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
