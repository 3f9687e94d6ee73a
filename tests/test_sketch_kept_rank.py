"""GPU parity of the tile kernels' sort where the in-bucket rank runs by position over the kept
keys: rows and counts bit-equal to the oracle's sketch_batch for single-tile records through
the P = 2048 kernel, with the number of kept keys (those in the buckets up to the one that
holds sorted position s - 1) placed at the rank's round boundaries (multiples of the 256
threads), without a cut, at s = 1, with a second pass, with a bucket long enough for the
bitonic path, and one multi-tile group through the survivors-only (THR) kernel.

Every case derives the property it is about from the oracle's hashes of its own input and
asserts it, so an input that stops hitting its boundary fails here instead of passing idle.
"""
import functools

import numpy as np
import pytest

from test_gpu_sketch_dispatch import (INVALID, rand_acgt, run_parity, survivors_group,
                                      window_keys)

pytestmark = pytest.mark.gpu

K = 21
LEN = 2000                      # 1,980 starts: one tile of the P = 2048 class
NB, SHIFT = 1024, 54            # the tile's buckets: the top 10 bits of a 64-bit key
MAX_BUCKET = 32                 # a longer bucket sends the tile to the bitonic sort
CLASS_2048 = [0, 0, 0, 1, 0, 0]


def _keys(oracle, seq):
    k = window_keys(oracle, seq, K)
    return k[k != INVALID]


def _kept(keys, s):
    """keys the first pass ranks at sketch size s: all of them without a cut, else those of
    the buckets up to the one holding sorted position s - 1"""
    if s > len(keys):
        return len(keys)
    b = np.sort(keys)[s - 1] >> np.uint64(SHIFT)
    return int(((keys >> np.uint64(SHIFT)) <= b).sum())


@functools.lru_cache(maxsize=None)
def _boundary_record(target):
    """(record, s): a random record one of whose bucket boundaries has exactly `target` keys
    below it; at s = target the first pass keeps exactly those"""
    from oracle import oracle as O
    O.lib()
    for seed in range(200):
        seq = rand_acgt(np.random.default_rng(7100 + 1000 * target + seed), LEN)
        keys = _keys(O, seq)
        cum = np.cumsum(np.bincount((keys >> np.uint64(SHIFT)).astype(np.int64), minlength=NB))
        if target in cum and len(np.unique(keys)) == len(keys):
            return seq, target
    raise AssertionError(f"no seed puts a bucket boundary at {target} keys")


@pytest.mark.parametrize("target", [255, 256, 257, 511, 512, 513, 1023, 1024, 1025])
def test_kept_keys_at_round_boundaries(ctx, oracle, target):
    seq, s = _boundary_record(target)
    keys = _keys(oracle, seq)
    assert _kept(keys, s) == target and len(keys) == LEN - K + 1
    plan, _ = run_parity(ctx, oracle, dict(k=K, s=s), [seq], what=f"kept={target}")
    assert plan["tiles"] == CLASS_2048


@pytest.mark.parametrize("s", [LEN, 1])
def test_no_cut_and_one(ctx, oracle, s):
    """s >= the windows: no cut, every round runs.  s = 1: the first non-empty bucket alone."""
    seq = rand_acgt(np.random.default_rng(7001), LEN)
    keys = _keys(oracle, seq)
    kept = _kept(keys, s)
    assert kept == len(keys) if s == LEN else 1 <= kept <= MAX_BUCKET
    plan, _ = run_parity(ctx, oracle, dict(k=K, s=s), [seq], what=f"s={s}")
    assert plan["tiles"] == CLASS_2048


def test_second_pass(ctx, oracle):
    """A record of three copies of one stretch: the kept buckets hold s keys but a third as
    many distinct values, so the buckets past the cut are ranked too."""
    rng = np.random.default_rng(7002)
    seq = rand_acgt(rng, 600) * 3 + rand_acgt(rng, 200)
    s = 500
    keys = _keys(oracle, seq)
    b = np.sort(keys)[s - 1] >> np.uint64(SHIFT)
    kept = keys[(keys >> np.uint64(SHIFT)) <= b]
    assert len(np.unique(kept)) < s <= len(np.unique(keys))
    assert np.bincount((keys >> np.uint64(SHIFT)).astype(np.int64)).max() <= MAX_BUCKET
    plan, _ = run_parity(ctx, oracle, dict(k=K, s=s), [seq], what="second pass")
    assert plan["tiles"] == CLASS_2048


def test_long_bucket_bitonic(ctx, oracle):
    """A run of one base: hundreds of copies of one key in one bucket."""
    rng = np.random.default_rng(7003)
    seq = rand_acgt(rng, 1000) + b"A" * 500 + rand_acgt(rng, 500)
    keys = _keys(oracle, seq)
    assert np.bincount((keys >> np.uint64(SHIFT)).astype(np.int64)).max() > MAX_BUCKET
    plan, _ = run_parity(ctx, oracle, dict(k=K, s=1000), [seq], what="long bucket")
    assert plan["tiles"] == CLASS_2048


def test_multi_tile_survivors_kernel(ctx, oracle):
    """The least group the survivors-only kernel takes at s = 1000 (32 chunks): its tiles rank
    by position with 4 slots per thread, the overflowing ones through the redo kernel."""
    rec, _bound, _keys_ = survivors_group(K, 1000, 32)
    plan, hooks = run_parity(ctx, oracle, dict(k=K, s=1000), [rec], [0], 1, what="thr")
    assert plan["tiles"] == [0, 0, 0, 0, 32, 0] and plan["thr4"] == 1
    assert hooks["redo"] > 0
