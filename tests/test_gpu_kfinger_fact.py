"""fpm_kfinger_* under fpm_kfinger_set_factorization against tests/kfinger_fact_model.py: for
ICFL and for CFL_ICFL at T = 10, 20, 30 and 1, the comparison of tests/test_gpu_kfinger.py, exact:
the line hashes (u32 and u64, seed 42 and another), the value counts, the record -> line map, the
values and the text.  Inputs are a few KB and are built in kfinger_fact_model, where
tests/test_kfinger_fact_model.py shows that each sits on the edge it is named for.  R is the run
length (window starts per workgroup) and KMAX the widest window, from fpm_kfinger_limits; LDSW is
the widest window whose ICFL working memory is in LDS (csrc/fpm_kernels.hpp: kKfLdsWindow), the
next one is the first to keep it in device memory."""
import ctypes as C

import numpy as np
import pytest

import fpmash
import kfinger_fact_model as F
import kfinger_model as M

pytestmark = pytest.mark.gpu

KMAX, R = fpmash.kfinger_limits()
LDSW = 192
SEEDS = (42, 7)


def check(ctx, oracle, seqs, w, fact, ids=None, max_lines=None, model=None):
    ids = F.default_ids(len(seqs)) if ids is None else ids
    m = model or F.Model(seqs, ids, w, fact, max_lines)
    for use64 in (False, True):
        for seed in SEEDS:
            r = ctx.kfinger(seqs, window=w, seed=seed, use64=use64, max_lines=max_lines, ids=ids,
                            values=True, text=True, factorization=fact)
            assert r["n_lines"] == len(m.lines)
            assert np.array_equal(r["rec_first_line"], m.rec_first_line)
            assert np.array_equal(r["n_vals"], m.n_vals)
            assert np.array_equal(r["val_off"], m.val_off)
            assert np.array_equal(r["vals"], m.flat)
            assert r["text"] == m.text
            assert r["hash"].dtype == (np.uint64 if use64 else np.uint32)
            assert np.array_equal(r["hash"], m.hashes(oracle, seed, use64))
    return m


@pytest.mark.parametrize("fact", F.FACTS)
@pytest.mark.parametrize("w", [100, 1, 2, 3, 17, LDSW, LDSW + 1, 255, 256])
def test_windows(ctx, oracle, w, fact):
    """the cyclic wrap, runs crossing workgroups and the short-record path, on either side of
    the window where the working memory leaves LDS"""
    seqs = F.window_seqs(w, R)
    m = check(ctx, oracle, seqs, w, fact)
    assert len(m.lines) == sum(M.n_lines(len(s), w) for s in seqs)


@pytest.mark.parametrize("fact", F.FACTS)
def test_widest_window(ctx, oracle, fact):
    """the model's lines come through cflgen here"""
    seqs = F.wide_seqs(KMAX, R)
    m = check(ctx, oracle, seqs, KMAX, fact,
              model=F.Model(seqs, F.default_ids(len(seqs)), KMAX, fact, fast=True))
    assert len(m.lines) == 1 + KMAX + KMAX + 1 + R + KMAX


@pytest.mark.parametrize("fact", F.FACTS)
@pytest.mark.parametrize("w", [99, 100, LDSW + 1])
def test_extremes(ctx, oracle, w, fact):
    """n - 1 steps, one factor, deep border chains, the merge branch, records of 1, 2 and 3
    bytes, both factor-count parities (the 8-byte Murmur tail); past LDSW the same in device
    memory"""
    m = check(ctx, oracle, F.EXTREMES, w, fact)
    if fact == "ICFL" and w == 100:
        first = int(m.rec_first_line[0])
        assert m.vals[first].tolist() == [1] * 100          # ascending: 99 steps
        assert m.vals[int(m.rec_first_line[1])].tolist() == [100]
        assert {int(v) & 1 for v in m.n_vals} == {0, 1}


@pytest.mark.parametrize("fact", F.FACTS)
def test_case_rule_unsigned_order_and_0x24(ctx, oracle, fact):
    """a-z fold to A-Z and nothing else does; bytes compare unsigned; 0x24 is a byte like any
    other (the expectation is the model's: lyn2vec's in-band '$' cannot take it)"""
    check(ctx, oracle, F.byte_rule_seqs(), 100, fact)


@pytest.mark.parametrize("T", [1, 10, 20, 30, 99])
def test_threshold_edge(ctx, oracle, T):
    """a Lyndon factor of exactly T bytes is kept, one of T + 1 is split"""
    seqs = [F.threshold_seq(T), b"A" + b"T" * (T - 1), b"A" + b"T" * T]
    if T == 99:
        seqs = seqs[1:]                                    # (the first is no short record)
    m = check(ctx, oracle, seqs, 100, "CFL_ICFL-%d" % T)
    assert m.vals[int(m.rec_first_line[len(seqs) - 2])].tolist() == [T]
    assert m.vals[int(m.rec_first_line[len(seqs) - 1])].tolist() == [1, T]


@pytest.mark.parametrize("fact", F.FACTS)
def test_max_lines_cuts_inside_a_run(ctx, oracle, fact):
    seqs = F.max_lines_seqs(R)
    total = 130 + 1 + R + 40 + 1
    for cap in (0, 70, 131 + R + 1, total + 5):
        m = check(ctx, oracle, seqs, 100, fact, max_lines=cap)
        assert len(m.lines) == min(cap, total)


@pytest.mark.parametrize("fact", F.FACTS)
@pytest.mark.parametrize("w", [100, LDSW + 1])
def test_jobs_without_lines(ctx, oracle, w, fact):
    """no record, records without a base, max_lines = 0, a take mask that drops every record:
    no line, empty outputs, in LDS and past LDSW (where a job with lines takes a working
    buffer and one without lines takes none)"""
    for seqs, cap in (([], None), ([b"", b""], None), ([F.rand(3, w + 5), b"AC"], 0)):
        m = check(ctx, oracle, seqs, w, fact, max_lines=cap)
        assert len(m.lines) == 0 and m.text == b""
        r = ctx.kfinger(seqs, window=w, ids=F.default_ids(len(seqs)), max_lines=cap, values=True,
                        text=True, factorization=fact)
        assert r["n_lines"] == 0 and r["text"] == b"" and len(r["vals"]) == 0
        assert r["rec_first_line"].tolist() == [0] * (len(seqs) + 1)
    image = b">a b\nACGTACGT\n>c d\nTTGA\n"
    d = ctx.kfinger_fasta([image], take=[0, 0], window=w, values=True, text=True, factorization=fact)
    assert d["n_lines"] == 0 and d["text"] == b"" and d["rec_first_line"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("fact", F.FACTS)
def test_many_short_records_share_a_workgroup(ctx, oracle, fact):
    many, mixed = F.short_record_sets()
    m = check(ctx, oracle, many, 100, fact)
    assert len(m.lines) == 300
    check(ctx, oracle, mixed, 100, fact)


@pytest.mark.parametrize("fact", F.FACTS)
def test_stage_seq_path(ctx, oracle, fact):
    """a FASTA image parsed on the device, with a take mask"""
    recs, take = F.stage_seq_records(R)
    image = b"".join(b">" + h + b"\n" + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60))
                     for h, s in recs)
    ids = [M.line_id(h) for h, _ in recs]
    kept = [s if t else b"" for (_, s), t in zip(recs, take)]
    m = F.Model(kept, ids, 100, fact)
    d = ctx.kfinger_fasta([image], take=take, window=100, values=True, text=True,
                          factorization=fact)
    assert d["text"] == m.text and np.array_equal(d["vals"], m.flat)
    assert np.array_equal(d["rec_first_line"], m.rec_first_line)
    assert np.array_equal(d["hash"], m.hashes(oracle, 42, False))


# ---- the C ABI call itself ------------------------------------------------------------------

def stage(ctx, seqs, w=100):
    data, off = fpmash.pack_records([bytes(s) for s in seqs])
    job, n = C.c_void_p(), C.c_uint64()
    fpmash._check(fpmash.lib().fpm_kfinger_stage(ctx.h, data, fpmash._p(off, fpmash.u64p), len(seqs),
                                                 w, 0xFFFFFFFFFFFFFFFF, C.byref(job), C.byref(n)))
    return job, n.value


def fetch(job, n):
    h = np.zeros(n, np.uint32)
    nv = np.zeros(n, np.uint32)
    fpmash._check(fpmash.lib().fpm_kfinger_fetch(job, None, h.ctypes.data, fpmash._p(nv, fpmash.u32p)))
    return h, nv


def test_abi_default_is_cfl_and_refusals(ctx, oracle):
    L = fpmash.lib()
    seqs = [F.rand(77, 180), b"CAACACC"]
    cfl = M.Model(seqs, F.default_ids(2), 100)
    icfl = F.Model(seqs, F.default_ids(2), 100, "ICFL")
    assert not np.array_equal(cfl.hashes(oracle, 42, False), icfl.hashes(oracle, 42, False))
    # a job that never makes the call, and one that asks for FPM_KF_CFL (its threshold ignored)
    for call in (False, True):
        job, n = stage(ctx, seqs)
        try:
            if call:
                assert L.fpm_kfinger_set_factorization(job, fpmash.KF_CFL, 12345678) == fpmash.FPM_OK
            fpmash._check(L.fpm_kfinger_run(job, 42, 0, None))
            h, nv = fetch(job, n)
            assert np.array_equal(h, cfl.hashes(oracle, 42, False)) and np.array_equal(nv, cfl.n_vals)
        finally:
            L.fpm_kfinger_free(job)
    # a bad kind, T = 0 and T past the widest window are refused and leave the job as it was:
    # ICFL (its threshold ignored too); after the run the call is refused and the job fetches
    job, n = stage(ctx, seqs)
    try:
        assert L.fpm_kfinger_set_factorization(job, fpmash.KF_ICFL, 0) == fpmash.FPM_OK
        for kind, thr in ((3, 10), (0xFFFFFFFF, 10), (fpmash.KF_CFL_ICFL, 0),
                          (fpmash.KF_CFL_ICFL, KMAX + 1)):
            assert L.fpm_kfinger_set_factorization(job, kind, thr) == fpmash.FPM_EINVAL
        assert L.fpm_kfinger_set_factorization(None, fpmash.KF_ICFL, 0) == fpmash.FPM_EINVAL
        fpmash._check(L.fpm_kfinger_run(job, 42, 0, None))
        for kind, thr in ((fpmash.KF_CFL, 0), (fpmash.KF_ICFL, 0), (fpmash.KF_CFL_ICFL, 10)):
            assert L.fpm_kfinger_set_factorization(job, kind, thr) == fpmash.FPM_EINVAL
        h, nv = fetch(job, n)
        assert np.array_equal(h, icfl.hashes(oracle, 42, False)) and np.array_equal(nv, icfl.n_vals)
    finally:
        L.fpm_kfinger_free(job)
    # the widest threshold is taken
    job, n = stage(ctx, seqs)
    try:
        assert L.fpm_kfinger_set_factorization(job, fpmash.KF_CFL_ICFL, KMAX) == fpmash.FPM_OK
        fpmash._check(L.fpm_kfinger_run(job, 42, 0, None))
        h, nv = fetch(job, n)
        assert np.array_equal(nv, cfl.n_vals)               # no factor is longer than KMAX
    finally:
        L.fpm_kfinger_free(job)


def test_binding_refuses_unknown_names(ctx):
    for name in ("FOO", "CFL_ICFL-0", "CFL_ICFL-%d" % (KMAX + 1)):
        with pytest.raises(ValueError):
            ctx.kfinger([b"ACGT"], factorization=name)
