"""SEED: the process-wide generators (D2 `seed_all_rng`) and the derivation of this project's own streams from (SEED, rank).

The streams are this project's, not the reference's: D2 draws its sampler seed from numpy on rank 0 and its mapper from numpy's
global state; here the index streams, the device mapper, the shrink-paste ratios and the label-sampling keys each own a generator
("Seeds and the reproducible step")."""
import os
import random
import time
from typing import Optional

import numpy as np
import torch

# stream ids: a trainer's generators are seeded with derive(SEED, rank, stream)
STREAM_RATIO, STREAM_KEYS = 1, 2


def seed_all_rng(seed: Optional[int] = None) -> int:
    """Seed Python `random`, numpy and torch (CPU and the current device).  None: a fresh seed from time, pid and os.urandom.
    Returns the seed used."""
    if seed is None:
        seed = (os.getpid() + int(time.time() * 1e6) % (1 << 31) + int.from_bytes(os.urandom(2), "big")) % (1 << 31)
    seed = int(seed)
    np.random.seed(seed % (1 << 32))
    torch.manual_seed(seed)                # (seeds the device generators as well, lazily where no device is initialised)
    random.seed(seed)
    return seed


def loader_seed(cfg, seed: Optional[int] = None) -> int:
    """The loader builders' `seed`: an explicit value as given, else cfg.SEED when it is >= 0, else 0"""
    if seed is not None:
        return int(seed)
    return int(cfg.SEED) if cfg.SEED >= 0 else 0


def derive(seed: int, rank: int, stream: int) -> int:
    """One 62-bit seed per (SEED, rank, stream): distinct streams for distinct triples in the ranges in use (rank < 2^16, stream < 2^8)"""
    return (int(seed) * 0x9E3779B1 + (int(rank) << 8) + int(stream)) % (1 << 62)
