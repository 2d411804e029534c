#!/usr/bin/env python
"""Are two builds of ptmi_conv3x3_wino4_wgrad the same function?  Runs both libraries on the test suite's WG_SHAPES and on the trainable
layer shapes (n = 2) with the same inputs and prints torch.equal of dW and db, for the plain entry point and for `waves` 3.
    python tools/exp/wino4w_bitident.py old.so new.so"""
import ctypes, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LAYERS = {"conv3_1": (128, 256, 200, 333), "conv3_2": (256, 256, 200, 333), "conv4_1": (256, 512, 100, 166),
          "conv4_2": (512, 512, 100, 166), "conv5_1": (512, 512, 50, 83)}


def main():
    from test_wino4_gpu import WG_SHAPES
    libs = [ctypes.CDLL(os.path.abspath(p)) for p in sys.argv[1:3]]
    for lib in libs:
        lib.ptmi_conv3x3_wino4_wgrad_ws_floats_waves.restype = ctypes.c_int64
    vp = ctypes.c_void_p
    shapes = list(WG_SHAPES) + [(2, cin, cout, h, w) for cin, cout, h, w in LAYERS.values()]
    bad = 0
    for n, cin, cout, h, w in shapes:
        gen = torch.Generator().manual_seed(n + cin + cout + h + w)
        x = torch.relu(torch.randn(n, cin, h, w, generator=gen)).to("cuda:0")
        dy = torch.randn(n, cout, h, w, generator=gen).to("cuda:0")
        for waves in (1, 3):
            outs = []
            for lib in libs:
                ws = torch.empty(lib.ptmi_conv3x3_wino4_wgrad_ws_floats_waves(n, cin, cout, h, w, waves), device="cuda:0")
                dw, db = torch.full((cout, cin, 3, 3), float("nan"), device="cuda:0"), torch.full((cout,), float("nan"), device="cuda:0")
                rc = lib.ptmi_conv3x3_wino4_wgrad_waves(vp(x.data_ptr()), vp(dy.data_ptr()), vp(dw.data_ptr()), vp(db.data_ptr()), vp(ws.data_ptr()),
                                                        n, cin, cout, h, w, 0, waves, vp(torch.cuda.current_stream().cuda_stream))
                assert rc == 0
                torch.cuda.synchronize()
                outs.append((dw, db))
            e_w, e_b = torch.equal(outs[0][0], outs[1][0]), torch.equal(outs[0][1], outs[1][1])
            fin = bool(torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all())
            bad += not (e_w and e_b and fin)
            print(f"n={n} cin={cin:3d} cout={cout:3d} {h:3d}x{w:<3d} waves={waves}  dW equal {e_w}  db equal {e_b}  finite {fin}", flush=True)
    print("all identical" if not bad else f"{bad} DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
