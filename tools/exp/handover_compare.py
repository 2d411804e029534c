#!/usr/bin/env python
"""Builds of libptmi355.so against each other in ONE process: the F(4x4,3x3) forward / dgrad kernel (csrc/wino4p.hip) and the weight
gradient (csrc/wino4w.hip).  The first library is the base of every comparison.

    python tools/exp/handover_compare.py time-fwd   --libs parent.so,new.so [--n 48] [--layers conv1_2,..] [--reps 2]
    python tools/exp/handover_compare.py time-wgrad --libs parent.so,new.so [--n 48] [--layers conv3_1,..] [--reps 2]
        every repetition walks the libraries in alternating order (a b, b a, ...); per library and layer: the ms of each repetition,
        the mean's ratio to the base, whether the outputs are the base's bits, and the job's repeat spread (max - min over the
        repetitions of one library, as a share of its min; the largest over libraries and layers is printed last).  A name may be
        given as name=path; elimination variants (tools/exp/make_wino4_variant.py) compute wrong numbers by design.
    python tools/exp/handover_compare.py bitident --libs parent.so,new.so
        torch.equal of forward (epilogues 0, 1, 4), dgrad (2, 3), both tile schedules, and of dW / db (waves 1, 3) on the shapes of
        tests/test_wino_handover_gpu.py and on the five VGG layer shapes at n = 16"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FWD_LAYERS = {"conv1_2": (64, 64, 800, 1333), "conv2_1": (64, 128, 400, 666), "conv2_2": (128, 128, 400, 666),
              "conv3_1": (128, 256, 200, 333), "conv3_2": (256, 256, 200, 333), "conv4_1": (256, 512, 100, 166),
              "conv4_2": (512, 512, 100, 166), "conv5_1": (512, 512, 50, 83)}
WG_LAYERS = {k: FWD_LAYERS[k] for k in ("conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5_1")}
VGG5 = ("conv1_2", "conv2_2", "conv3_2", "conv4_2", "conv5_1")
vp = ctypes.c_void_p
DEV = "cuda:0"


def load(spec):
    libs = []
    for item in spec.split(","):
        name, path = item.split("=") if "=" in item else (os.path.basename(item), item)
        lib = ctypes.CDLL(os.path.abspath(path))
        for f in ("ptmi_conv3x3_wino4p_packed_floats", "ptmi_conv3x3_wino4_wgrad_ws_floats_waves"):
            getattr(lib, f).restype = ctypes.c_int64
        libs.append((name, lib))
    return libs


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def rand(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV)


def fwd_call(lib, x, wt, bias, mask, epi, mode, sched=None):
    """pack + launch; -> y.  mode 1 (dgrad): x is dY [n, cout, h, w] and the result has wt.shape[1] channels"""
    co, ci = wt.shape[0], wt.shape[1]
    ccin, ccout = (ci, co) if mode == 0 else (co, ci)
    n, _, h, w = x.shape
    wp = torch.empty(lib.ptmi_conv3x3_wino4p_packed_floats(ccin, ccout), device=DEV)
    assert lib.ptmi_conv3x3_wino4p_pack_weights(vp(wt.data_ptr()), vp(wp.data_ptr()), co, ci, mode, stream()) == 0
    y = torch.full((n, ccout, h // 2, w // 2) if epi == 4 else (n, ccout, h, w), float("nan"), device=DEV)
    args = (vp(x.data_ptr()), vp(wp.data_ptr()), vp(bias.data_ptr() if bias is not None else None),
            vp(mask.data_ptr() if mask is not None else None), vp(y.data_ptr()), n, ccin, ccout, h, w, epi)
    if sched is None:
        rc = lib.ptmi_conv3x3_wino4p_fwd(*args, stream())
    else:
        rc = lib.ptmi_conv3x3_wino4p_fwd_sched(*args, vp(sched.data_ptr()), stream())
    assert rc == 0
    return y


def wgrad_call(lib, x, dy, waves, out=None):
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    if out is None:
        out = (torch.full((cout, cin, 3, 3), float("nan"), device=DEV), torch.full((cout,), float("nan"), device=DEV),
               torch.empty(lib.ptmi_conv3x3_wino4_wgrad_ws_floats_waves(n, cin, cout, h, w, waves), device=DEV))
    dw, db, ws = out
    assert lib.ptmi_conv3x3_wino4_wgrad_waves(vp(x.data_ptr()), vp(dy.data_ptr()), vp(dw.data_ptr()), vp(db.data_ptr()),
                                              vp(ws.data_ptr()), n, cin, cout, h, w, 0, waves, stream()) == 0
    return out


def timed(f, iters):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_mode(a, libs, wgrad):
    layers = WG_LAYERS if wgrad else FWD_LAYERS
    worst = 0.0
    for name in (a.layers.split(",") if a.layers else layers):
        cin, cout, h, w = layers[name]
        gen = torch.Generator(device=DEV).manual_seed(1)
        x = torch.relu(rand(gen, a.n, cin, h, w))
        runs, outs = [], []
        if wgrad:
            dy = rand(gen, a.n, cout, h, w)
            for _, lib in libs:
                o = wgrad_call(lib, x, dy, 1)
                outs.append(o)
                runs.append(lambda lib=lib, o=o: wgrad_call(lib, x, dy, 1, o))
        else:
            wt = rand(gen, cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5
            b = torch.zeros(cout, device=DEV)
            y = torch.empty(a.n, cout, h, w, device=DEV)
            for _, lib in libs:
                wp = torch.empty(lib.ptmi_conv3x3_wino4p_packed_floats(cin, cout), device=DEV)
                lib.ptmi_conv3x3_wino4p_pack_weights(vp(wt.data_ptr()), vp(wp.data_ptr()), cout, cin, 0, stream())

                def f(lib=lib, wp=wp):
                    assert lib.ptmi_conv3x3_wino4p_fwd(vp(x.data_ptr()), vp(wp.data_ptr()), vp(b.data_ptr()), vp(x.data_ptr()), vp(y.data_ptr()),
                                                       a.n, cin, cout, h, w, a.epi, stream()) == 0
                runs.append(f)
                f()
                outs.append((y[:1].clone(), y[-1:].clone()))         # (the whole tensors: the bitident mode)
        ms = [[] for _ in libs]
        for rep in range(a.reps):
            order = range(len(libs)) if rep % 2 == 0 else reversed(range(len(libs)))
            for i in order:
                ms[i].append(timed(runs[i], a.iters))
        base = sum(ms[0]) / len(ms[0])
        for i, (lname, _) in enumerate(libs):
            mean = sum(ms[i]) / len(ms[i])
            spread = (max(ms[i]) - min(ms[i])) / min(ms[i])
            worst = max(worst, spread)
            same = all(torch.equal(p, q) for p, q in zip(outs[0][:2], outs[i][:2]))
            print(f"{name:8s} n={a.n:2d} {lname:28s} " + " ".join(f"{t:8.4f}" for t in ms[i]) + f" ms  mean {mean:8.4f}  x{mean / base:.4f} of base"
                  f"  ({(mean / base - 1) * 100:+.2f} %)  repeat spread {spread * 100:.2f} %  same bits as base {same}", flush=True)
    print(f"largest repeat spread of one library on one layer in this job: {worst * 100:.2f} %")


def bitident(libs):
    from test_wino_handover_gpu import FWD_SHAPES, WG_SHAPES
    (_, old), (_, new) = libs[:2]
    bad = 0
    sched = torch.zeros(16, dtype=torch.int32, device=DEV)
    fwd = [(s, "test") for s in FWD_SHAPES] + [((16,) + FWD_LAYERS[k], k) for k in VGG5]
    for (n, cin, cout, h, w), tag in fwd:
        gen = torch.Generator(device=DEV).manual_seed(n + cin + cout + h + w)
        x, gy, mask = torch.relu(rand(gen, n, cin, h, w)), rand(gen, n, cout, h, w), rand(gen, n, cin, h, w)
        wt, b = rand(gen, cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, rand(gen, cout) * 0.1
        res = []
        for sc in (None, sched):
            for epi in (0, 1, 4, 2, 3):
                args = (x, wt, b, None, epi, 0) if epi in (0, 1, 4) else (gy, wt, None, mask if epi == 3 else None, epi, 1)
                yo = fwd_call(old, *args, sched=sc)
                yn = fwd_call(new, *args, sched=sc)
                ok = torch.equal(yo, yn) and bool(torch.isfinite(yn).all())
                bad += not ok
                res.append(f"{'dyn' if sc is not None else 'stat'}/{epi}:{'equal' if ok else 'DIFFER'}")
                del yo, yn
        print(f"fwd/dgrad {tag:8s} n={n} {cin}->{cout} {h}x{w}  " + " ".join(res), flush=True)
    wg = [(s, "test") for s in WG_SHAPES] + [((16,) + WG_LAYERS[k], k) for k in WG_LAYERS]
    for (n, cin, cout, h, w), tag in wg:
        gen = torch.Generator(device=DEV).manual_seed(n + cin + cout + h + w)
        x, dy = torch.relu(rand(gen, n, cin, h, w)), rand(gen, n, cout, h, w)
        res = []
        for waves in (1, 3):
            o, nw = wgrad_call(old, x, dy, waves), wgrad_call(new, x, dy, waves)
            ok = torch.equal(o[0], nw[0]) and torch.equal(o[1], nw[1]) and bool(torch.isfinite(nw[0]).all() and torch.isfinite(nw[1]).all())
            bad += not ok
            res.append(f"waves {waves}: dW, db {'equal' if ok else 'DIFFER'}")
        print(f"wgrad     {tag:8s} n={n} {cin}->{cout} {h}x{w}  " + "  ".join(res), flush=True)
    print("all identical" if not bad else f"{bad} DIFFER")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time-fwd", "time-wgrad", "bitident"])
    ap.add_argument("--libs", required=True)
    ap.add_argument("--n", type=int, default=48)
    ap.add_argument("--layers", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--epi", type=int, default=1)
    a = ap.parse_args()
    libs = load(a.libs)
    if a.mode == "bitident":
        return bitident(libs)
    time_mode(a, libs, a.mode == "time-wgrad")
    return 0


if __name__ == "__main__":
    sys.exit(main())
