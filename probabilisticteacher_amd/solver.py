"""LR schedules and optimiser options of the reference, as pure functions of the iteration.

Reference: pt/solver/build.py:22-57 (`build_lr_scheduler`: WarmupMultiStepLR, WarmupCosineLR [detectron2 0.5] and the
repo's own WarmupTwoStageMultiStepLR, pt/solver/lr_scheduler.py:22-66), driven by `hooks.LRScheduler`
(pt/engine/trainer.py:505).  The fused clip+SGD kernel takes the learning rate as a launch argument, so a schedule is
just `lr(it)`; there is no scheduler object to step.  torch.optim.SGD options the reference leaves at their defaults
(D2 build_optimizer: per-parameter groups with BIAS_LR_FACTOR / WEIGHT_DECAY_BIAS / WEIGHT_DECAY_NORM, NESTEROV) are
checked, not silently ignored."""
import bisect
import math


def warmup_factor_at_iter(method: str, it: int, warmup_iters: int, warmup_factor: float) -> float:
    """detectron2 `_get_warmup_factor_at_iter`."""
    if it >= warmup_iters:
        return 1.0
    if method == "constant":
        return warmup_factor
    if method == "linear":
        alpha = it / warmup_iters
        return warmup_factor * (1 - alpha) + alpha
    raise ValueError("Unknown warmup method: {}".format(method))


def lr_at(cfg, it: int) -> float:
    """Learning rate used by iteration `it` (== scheduler.get_lr() with last_epoch == it)."""
    S = cfg.SOLVER
    name = S.LR_SCHEDULER_NAME
    warm = warmup_factor_at_iter(S.WARMUP_METHOD, it, S.WARMUP_ITERS, S.WARMUP_FACTOR)
    if name == "WarmupMultiStepLR":
        return S.BASE_LR * warm * S.GAMMA ** bisect.bisect_right(list(S.STEPS), it)
    if name == "WarmupCosineLR":
        return S.BASE_LR * warm * 0.5 * (1.0 + math.cos(math.pi * it / S.MAX_ITER))
    if name == "WarmupTwoStageMultiStepLR":
        steps, factors = list(S.STEPS), list(S.FACTOR_LIST)
        if steps != sorted(steps):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(steps))
        if len(steps) + 1 != len(factors):
            raise ValueError("Length of milestones should match length of factor_list.")
        return S.BASE_LR * warm * factors[bisect.bisect_right(steps, it)]
    raise ValueError("Unknown LR scheduler: {}".format(name))


def check_optimizer_options(cfg) -> None:
    """The fused step implements torch.optim.SGD(momentum, weight_decay) with one setting for every parameter -- what the
    shipped configs select.  Anything else must fail loudly instead of training with the wrong optimiser."""
    S = cfg.SOLVER
    if S.NESTEROV:
        raise ValueError("SOLVER.NESTEROV=True is not implemented by the fused clip+SGD step")
    if float(S.BIAS_LR_FACTOR) != 1.0:
        raise ValueError("SOLVER.BIAS_LR_FACTOR != 1 is not implemented by the fused clip+SGD step")
    if float(S.WEIGHT_DECAY_BIAS) != float(S.WEIGHT_DECAY):
        raise ValueError("SOLVER.WEIGHT_DECAY_BIAS != SOLVER.WEIGHT_DECAY is not implemented by the fused clip+SGD step")
    weight_decay_norm(cfg)
    clip_gradients_options(cfg)
    lr_at(cfg, 0)         # unknown scheduler / warm-up names raise here, before the first step


def weight_decay_norm(cfg) -> float:
    """SOLVER.WEIGHT_DECAY_NORM (D2 get_default_optimizer_params: the weight decay of the parameters of norm modules; every
    other parameter gets WEIGHT_DECAY): any finite value >= 0.  The fused step reads it from a per-segment table."""
    try:
        value = float(cfg.SOLVER.WEIGHT_DECAY_NORM)
    except (TypeError, ValueError):
        value = float("nan")
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f"SOLVER.WEIGHT_DECAY_NORM must be a finite number >= 0, got {cfg.SOLVER.WEIGHT_DECAY_NORM!r}")
    return value


def norm_parameter_names(model) -> set:
    """Names (as `model.named_parameters()` gives them) of the parameters D2's get_default_optimizer_params treats as norm
    parameters: those that belong to a norm module directly.  Here the norm modules are the `norm` children of the backbone's
    and the box head's convolutions (modeling/backbone.py: _GroupNormParams)."""
    from .modeling.backbone import _GroupNormParams
    names = set()
    for mod_name, mod in model.named_modules():
        if isinstance(mod, _GroupNormParams):
            names.update(f"{mod_name}.{n}" if mod_name else n for n, _ in mod.named_parameters(recurse=False))
    return names


def segment_weight_decay(cfg, model, names) -> list:
    """[weight decay of parameter `n` for n in names]: WEIGHT_DECAY_NORM for norm parameters, WEIGHT_DECAY for the others"""
    norm = norm_parameter_names(model)
    wd, wdn = float(cfg.SOLVER.WEIGHT_DECAY), weight_decay_norm(cfg)
    return [wdn if n in norm else wd for n in names]


def clip_gradients_options(cfg):
    """SOLVER.CLIP_GRADIENTS as the fused step takes it: None when disabled (D2 0.5 does not look at the other three keys
    then), else (clip_type "value" | "norm", clip_value > 0, inf_norm).  D2 accepts any NORM_TYPE torch does; the segment-norm
    kernel implements 2.0 and inf (float, or the string "inf" a YAML file or a command-line override delivers)."""
    G = cfg.SOLVER.CLIP_GRADIENTS
    if not G.ENABLED:
        return None
    if G.CLIP_TYPE not in ("value", "norm"):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE must be 'value' or 'norm' (per-parameter clipping), got {G.CLIP_TYPE!r}")
    try:
        value = float(G.CLIP_VALUE)
    except (TypeError, ValueError):
        value = float("nan")
    if not value > 0.0:
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_VALUE must be > 0, got {G.CLIP_VALUE!r}")
    try:
        norm_type = float(G.NORM_TYPE)
    except (TypeError, ValueError):
        norm_type = float("nan")
    if norm_type not in (2.0, math.inf):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE must be 2.0 or inf, got {G.NORM_TYPE!r}")
    return G.CLIP_TYPE, value, norm_type == math.inf


def scheduler_state(cfg, last_iter: int, n_groups: int = 1) -> dict:
    """state_dict of the reference's `_LRScheduler` after finishing iteration `last_iter` (what fvcore's Checkpointer
    stores under "scheduler"); only `last_epoch` carries information."""
    nxt = last_iter + 1
    return {"last_epoch": nxt, "_step_count": nxt + 1, "base_lrs": [cfg.SOLVER.BASE_LR] * n_groups,
            "_last_lr": [lr_at(cfg, nxt)] * n_groups}
