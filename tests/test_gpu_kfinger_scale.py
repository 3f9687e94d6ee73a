"""fpm_kfinger_* where the size of the job changes what runs, exact like tests/test_gpu_kfinger.py
and tests/test_gpu_kfinger_fact.py.

Grid stride: past LDSW, the widest window whose ICFL working memory is in LDS (csrc/
fpm_kernels.hpp: kKfLdsWindow), a grid of G = two workgroups per compute unit shares the job's
descriptors out, workgroup g taking g, g + G, ... and reusing its stage and its region of the
working buffer for each.  G comes from fpm_kfinger_wide_groups on a job of many one-pack
descriptors; the job under test has 2 G + 37 of them, so workgroups take three or two.

Scan: at window 2 a record of more than F * B bytes (B, F: fpm_scan_limits) makes as many
lines, and the scans of the values pass and of the text pass take their three-launch form
inside fpm_kfinger_values / fpm_kfinger_text, which size the scratch themselves.
"""
import ctypes as C

import numpy as np
import pytest

import fpmash
import kfinger_fact_model as FM
import kfinger_model as M
from test_gpu_kfinger_fact import LDSW, check, stage

pytestmark = pytest.mark.gpu

KMAX, R = fpmash.kfinger_limits()
STAGE = R + KMAX - 1            # bytes of short records one descriptor packs at most
B, F = fpmash.scan_limits()
W = LDSW + 1
FACTS = ("ICFL", "CFL_ICFL-30")
PROBE_DESCS = 1500


@pytest.fixture(scope="module")
def groups(ctx):
    """G: the workgroups of a wide-window grid on this device.  First the descriptor count of
    kfinger_fact_model.plan_descs is shown to be the library's, on jobs with fewer descriptors
    than G (their grid has one workgroup per descriptor); then a job of PROBE_DESCS packs of
    short records reads G."""
    for n_desc in (1, 60):
        seqs = FM.stride_seqs(n_desc, W, R)
        assert FM.plan_descs([len(s) for s in seqs], W, R, STAGE) == n_desc
        assert ctx.kfinger(seqs, window=W, factorization="ICFL")["wide_groups"] == n_desc
    # the hook says 0 where no such grid runs: CFL, and the widest window kept in LDS
    assert ctx.kfinger(seqs, window=W)["wide_groups"] == 0
    assert ctx.kfinger(seqs, window=LDSW, factorization="ICFL")["wide_groups"] == 0
    # ... and before the run
    L = fpmash.lib()
    job, _ = stage(ctx, seqs, W)
    try:
        g = C.c_uint32(7)
        fpmash._check(L.fpm_kfinger_set_factorization(job, fpmash.KF_ICFL, 0))
        assert L.fpm_kfinger_wide_groups(job, C.byref(g)) == fpmash.FPM_OK and g.value == 0
        assert L.fpm_kfinger_wide_groups(job, None) == fpmash.FPM_EINVAL
        assert L.fpm_kfinger_wide_groups(None, C.byref(g)) == fpmash.FPM_EINVAL
        fpmash._check(L.fpm_kfinger_run(job, 42, 0, None))
        assert L.fpm_kfinger_wide_groups(job, C.byref(g)) == fpmash.FPM_OK and g.value == 60
    finally:
        L.fpm_kfinger_free(job)
    per_pack = STAGE // (W - 1)
    seqs = [FM.rand(5, W - 1)] * (per_pack * PROBE_DESCS)
    assert FM.plan_descs([W - 1] * len(seqs), W, R, STAGE) == PROBE_DESCS
    g = ctx.kfinger(seqs, window=W, factorization="ICFL")["wide_groups"]
    assert 0 < g < PROBE_DESCS and g % 2 == 0, "the device takes more workgroups than the probe has"
    return g


@pytest.fixture(scope="module")
def stride_job(groups):
    seqs = FM.stride_seqs(2 * groups + 37, W, R)
    return seqs, FM.default_ids(len(seqs)), {}


def stride_model(stride_job, fact):
    seqs, ids, models = stride_job
    if fact not in models:
        models[fact] = FM.Model(seqs, ids, W, fact, fast=True)
    return models[fact]


@pytest.mark.parametrize("fact", FACTS)
def test_grid_stride(ctx, oracle, groups, stride_job, fact):
    """2 G + 37 descriptors of both kinds: the first 37 workgroups take three, the others two"""
    seqs, ids, _ = stride_job
    n_desc = FM.plan_descs([len(s) for s in seqs], W, R, STAGE)
    assert n_desc == 2 * groups + 37 and 2 * groups < n_desc < 3 * groups
    m = stride_model(stride_job, fact)
    assert len(m.lines) == sum(M.n_lines(len(s), W) for s in seqs)
    check(ctx, oracle, seqs, W, fact, ids=ids, model=m)
    r = ctx.kfinger(seqs, window=W, factorization=fact)
    assert r["wide_groups"] == groups < n_desc


@pytest.mark.parametrize("fact", FACTS)
def test_grid_stride_cut_by_max_lines(ctx, oracle, groups, stride_job, fact):
    """the same job ended inside a run of its last third: fewer descriptors, so workgroups take
    two or one, and the last descriptor is short"""
    seqs, ids, _ = stride_job
    m = stride_model(stride_job, fact)
    lens = [len(s) for s in seqs]
    # 100 lines into the last long record that starts in the first five sixths of the lines
    rec = max(r for r, n in enumerate(lens)
              if n >= W and m.rec_first_line[r] <= len(m.lines) * 5 // 6)
    cap = int(m.rec_first_line[rec]) + 100
    n_desc = FM.plan_descs(lens, W, R, STAGE, cap)
    assert len(m.lines) * 2 // 3 < cap < len(m.lines)
    assert groups < n_desc < 2 * groups + 37
    c = FM.cut(m, cap)
    assert len(c.lines) == cap
    check(ctx, oracle, seqs, W, fact, ids=ids, max_lines=cap, model=c)
    r = ctx.kfinger(seqs, window=W, factorization=fact, max_lines=cap)
    assert r["wide_groups"] == groups < n_desc


# ---- more lines than the scan's two-launch form takes --------------------------------------

@pytest.fixture(scope="module")
def long_record():
    n = F * B + B + 1
    rng = np.random.default_rng(2)
    seq = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), size=n,
                     p=[.22, .22, .22, .22, .03, .03, .03, .03])
    seq = seq.tobytes()
    return seq, M.window2(seq, b"g")


@pytest.mark.parametrize("use64", [False, True])
def test_scans_of_both_passes_past_the_fold(ctx, oracle, long_record, use64):
    seq, want = long_record
    assert len(seq) > F * B                      # one line per byte: three-launch scans
    assert 0 < want["rising"].sum() < len(seq) and any(c in seq for c in b"acgt")
    r = ctx.kfinger([seq], window=2, seed=42, use64=use64, ids=[b"g"], values=True, text=True)
    assert r["n_lines"] == len(seq) and r["rec_first_line"].tolist() == [0, len(seq)]
    assert r["wide_groups"] == 0
    assert np.array_equal(r["n_vals"], want["n_vals"])
    bad = np.nonzero(r["val_off"] != want["val_off"])[0]
    assert len(bad) == 0, f"val_off differs first at line {bad[:1]}"
    assert np.array_equal(r["vals"], want["vals"])
    assert r["text"] == want["text"]
    h2, h11 = oracle.get_hash_fp([2], 42, use64), oracle.get_hash_fp([1, 1], 42, use64)
    assert h2 != h11
    dt = np.uint64 if use64 else np.uint32
    assert r["hash"].dtype == dt
    assert np.array_equal(r["hash"], np.where(want["rising"], dt(h2), dt(h11)))
