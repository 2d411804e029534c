#!/usr/bin/env python
"""tools/gen_golden_laplace.py -- DEV-CONTAINER ONLY.  Reference fixtures of the Laplace uncertainty model.

Drives the same reference code paths as tools/gen_golden.py (same stubs, seeds and inputs), with the reference
config's UNSUPNET.MODEL_TYPE set to "LAPLACE", and writes

    tests/golden/model_laplace_diff_anchor.npz      supervised / teacher / unsupervised branches (+ anchor gradient)
    tests/golden/model_laplace_default_anchor.npz   the same with the fixed anchor generator
    tests/golden/run_step_laplace.npz               three real PTrainer.run_step iterations

tools/gen_golden.py itself is untouched, so the Gaussian fixtures keep regenerating byte for byte.

    python tools/gen_golden_laplace.py            # [model] [step] to write a subset
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden  # noqa: E402

_build_cfg = gen_golden.build_cfg
_save = gen_golden.save


def build_cfg_laplace(*a, **k):
    cfg = _build_cfg(*a, **k)
    cfg.UNSUPNET.MODEL_TYPE = "LAPLACE"
    return cfg


def save_laplace(name, **arrs):
    # gen_run_step hard-codes its fixture name; map it here so the Gaussian run_step.npz is never written
    _save({"run_step": "run_step_laplace"}.get(name, name), **arrs)


def main():
    gen_golden.install_stubs()
    torch.Tensor.cuda = lambda self, *a, **k: self   # anchor_generator.py:69 hard-codes .cuda()
    torch.set_num_threads(8)
    gen_golden.build_cfg = build_cfg_laplace
    gen_golden.save = save_laplace
    which = sys.argv[1:] or ["model", "step"]
    if "model" in which:
        gen_golden.gen_model_branches("DifferentiableAnchorGenerator", "laplace_diff_anchor")
        gen_golden.gen_model_branches("DefaultAnchorGenerator", "laplace_default_anchor")
    if "step" in which:
        gen_golden.gen_run_step()


if __name__ == "__main__":
    main()
