"""fpm_kfinger_* under fpm_kfinger_set_comb against tests/kfinger_comb_model.py: for CFL_COMB,
ICFL_COMB and CFL_ICFL_COMB at T = 10 and 40, the comparison of tests/test_gpu_kfinger_fact.py,
exact: the line hashes (u32 and u64, seed 42 and another), the value counts, the record -> line
map, the values and the text.  Inputs are a few KB and are built in kfinger_comb_model and
kfinger_fact_model, where tests/test_kfinger_comb_model.py shows that each sits on the edge it is
named for.  R is the run length (window starts per workgroup) and KMAX the widest window, from
fpm_kfinger_limits; K.lds_window(fact) is the widest window whose working memory is in LDS, from
fpm_kfinger_lds_window, and the next one is the first to keep it in device memory."""
import ctypes as C

import numpy as np
import pytest

import fpmash
import kfinger_comb_model as K
import kfinger_fact_model as F
import kfinger_model as M
from test_gpu_kfinger_fact import check, fetch, stage

pytestmark = pytest.mark.gpu

KMAX, R = fpmash.kfinger_limits()
WINDOWS = [100, 1, 2, 3, 17, "lds", "lds+1", 255, 256]


def window_of(w, fact):
    return {"lds": K.lds_window(fact), "lds+1": K.lds_window(fact) + 1}.get(w, w)


@pytest.mark.parametrize("fact", K.FACTS)
@pytest.mark.parametrize("w", WINDOWS)
def test_windows(ctx, oracle, w, fact):
    """the cyclic wrap, runs crossing workgroups and the short-record path, on either side of
    the window where the working memory leaves LDS and where u8 entries end"""
    w = window_of(w, fact)
    seqs = F.window_seqs(w, R)
    m = check(ctx, oracle, seqs, w, fact)
    assert len(m.lines) == sum(M.n_lines(len(s), w) for s in seqs)
    r = ctx.kfinger(seqs, window=w, factorization=fact)
    assert (r["wide_groups"] > 0) == (w > K.lds_window(fact))


@pytest.mark.parametrize("fact", K.FACTS)
def test_widest_window(ctx, oracle, fact):
    """the model's lines come through cflgen here"""
    seqs = F.wide_seqs(KMAX, R)
    m = check(ctx, oracle, seqs, KMAX, fact,
              model=K.Model(seqs, K.default_ids(len(seqs)), KMAX, fact, fast=True))
    assert len(m.lines) == 1 + KMAX + KMAX + 1 + R + KMAX


@pytest.mark.parametrize("fact", K.FACTS)
@pytest.mark.parametrize("w", [4, 100, "lds+1"])
def test_records_shorter_than_the_window(ctx, oracle, w, fact):
    """records of 1, 2 and w - 1 bytes: the mirror runs over the line's own length"""
    w = window_of(w, fact)
    seqs = K.short_record_seqs(w)
    assert [len(s) for s in seqs[1:4]] == [1, 2, w - 1]
    check(ctx, oracle, seqs, w, fact)


@pytest.mark.parametrize("fact", K.FACTS)
def test_byte_rules_and_own_reverse_complements(ctx, oracle, fact):
    """lower case, N, an IUPAC code, 0x24 and bytes >= 0x80 in one record: a-z fold, A <-> T
    and C <-> G complement, every other byte is its own complement; then words equal to their
    reverse complement, whose two sides share every cut"""
    check(ctx, oracle, K.byte_rule_seqs() + K.own_reverse_complements() + F.EXTREMES, 100, fact)


@pytest.mark.parametrize("fact", K.FACTS)
def test_max_lines_cuts_inside_a_run(ctx, oracle, fact):
    seqs = F.max_lines_seqs(R)
    total = 130 + 1 + R + 40 + 1
    whole = K.Model(seqs, K.default_ids(len(seqs)), 100, fact)
    for cap in (0, 70, 131 + R + 1, total + 5):
        m = check(ctx, oracle, seqs, 100, fact, max_lines=cap, model=F.cut(whole, cap))
        assert len(m.lines) == min(cap, total)


@pytest.mark.parametrize("fact", K.FACTS)
@pytest.mark.parametrize("w", [100, "lds+1"])
def test_jobs_without_lines(ctx, oracle, w, fact):
    """no record, records without a base, max_lines = 0, a take mask that drops every record,
    at an LDS window and at a wide one (where a job with lines takes a working buffer and one
    without lines takes none)"""
    w = window_of(w, fact)
    for seqs, cap in (([], None), ([b"", b""], None), ([F.rand(3, w + 5), b"AC"], 0)):
        r = ctx.kfinger(seqs, window=w, ids=K.default_ids(len(seqs)), max_lines=cap, values=True,
                        text=True, factorization=fact)
        assert r["n_lines"] == 0 and r["text"] == b"" and len(r["vals"]) == 0
        assert r["rec_first_line"].tolist() == [0] * (len(seqs) + 1)
        assert r["wide_groups"] == 0
    image = b">a b\nACGTACGT\n>c d\nTTGA\n"
    d = ctx.kfinger_fasta([image], take=[0, 0], window=w, values=True, text=True, factorization=fact)
    assert d["n_lines"] == 0 and d["text"] == b"" and d["rec_first_line"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("fact", K.FACTS)
def test_many_short_records_share_a_workgroup(ctx, oracle, fact):
    many, mixed = F.short_record_sets()
    m = check(ctx, oracle, many, 100, fact)
    assert len(m.lines) == 300
    check(ctx, oracle, mixed, 100, fact)


@pytest.mark.parametrize("fact", K.FACTS)
def test_stage_seq_path(ctx, oracle, fact):
    """a FASTA image parsed on the device, with a take mask"""
    recs, take = F.stage_seq_records(R)
    image = b"".join(b">" + h + b"\n" + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60))
                     for h, s in recs)
    ids = [M.line_id(h) for h, _ in recs]
    kept = [s if t else b"" for (_, s), t in zip(recs, take)]
    m = K.Model(kept, ids, 100, fact)
    d = ctx.kfinger_fasta([image], take=take, window=100, values=True, text=True,
                          factorization=fact)
    assert d["text"] == m.text and np.array_equal(d["vals"], m.flat)
    assert np.array_equal(d["rec_first_line"], m.rec_first_line)
    assert np.array_equal(d["hash"], m.hashes(oracle, 42, False))


STAGE = R + KMAX - 1            # bytes of short records one descriptor packs at most
PROBE_DESCS = 1500


@pytest.fixture(scope="module")
def groups(ctx):
    """G: the workgroups of a wide-window grid on this device (two per compute unit), read from
    a job of PROBE_DESCS one-pack descriptors as tests/test_gpu_kfinger_scale.py reads it"""
    w = K.lds_window("CFL_COMB") + 1
    seqs = [F.rand(5, w - 1)] * (STAGE // (w - 1) * PROBE_DESCS)
    assert F.plan_descs([w - 1] * len(seqs), w, R, STAGE) == PROBE_DESCS
    g = ctx.kfinger(seqs, window=w, factorization="CFL_COMB")["wide_groups"]
    assert 0 < g < PROBE_DESCS and g % 2 == 0, "the device takes more workgroups than the probe has"
    return g


@pytest.mark.parametrize("fact", K.FACTS)
def test_wide_regions_are_reused_by_the_grid_stride_loop(ctx, oracle, groups, fact):
    """one wide-mode job of 2 G + 37 descriptors of both kinds: the first 37 workgroups take
    three, the others two, and every line clears its cut bits in a region lines before it used"""
    w = K.lds_window(fact) + 1
    n_desc = 2 * groups + 37
    seqs = K.stride_seqs(n_desc, w, R, STAGE)
    assert F.plan_descs([len(s) for s in seqs], w, R, STAGE) == n_desc
    ids = K.default_ids(len(seqs))
    m = check(ctx, oracle, seqs, w, fact, ids=ids, model=K.Model(seqs, ids, w, fact, fast=True))
    assert len(m.lines) == sum(M.n_lines(len(s), w) for s in seqs)
    r = ctx.kfinger(seqs, window=w, factorization=fact)
    assert r["wide_groups"] == groups < n_desc


# ---- the C ABI call itself ------------------------------------------------------------------

def run_job(ctx, oracle, seqs, model, calls):
    """stage, make `calls` (name, args, expected status) on the job, run, compare with model"""
    L = fpmash.lib()
    job, n = stage(ctx, seqs)
    try:
        for name, args, want in calls:
            assert getattr(L, name)(job, *args) == want, (name, args)
        fpmash._check(L.fpm_kfinger_run(job, 42, 0, None))
        h, nv = fetch(job, n)
        assert np.array_equal(h, model.hashes(oracle, 42, False))
        assert np.array_equal(nv, model.n_vals)
        return job
    except BaseException:
        L.fpm_kfinger_free(job)
        raise


def test_abi_default_is_not_combined_and_refusals(ctx, oracle):
    L = fpmash.lib()
    OK, EINVAL = fpmash.FPM_OK, fpmash.FPM_EINVAL
    seqs = [F.rand(77, 180), b"CAACACC", b"AGTCA"]
    ids = K.default_ids(3)
    kinds = {"CFL": (fpmash.KF_CFL, 0), "ICFL": (fpmash.KF_ICFL, 0),
             "CFL_ICFL-10": (fpmash.KF_CFL_ICFL, 10)}
    for name, (kind, thr) in kinds.items():
        plain = F.Model(seqs, ids, 100, name)
        comb = K.Model(seqs, ids, 100, name.replace("CFL_ICFL-", "CFL_ICFL_COMB-")
                       if "-" in name else name + "_COMB")
        assert not np.array_equal(plain.n_vals, comb.n_vals)
        setf = ("fpm_kfinger_set_factorization", (kind, thr), OK)
        # a job that never makes the call, and one that makes it with 0, give today's lines
        L.fpm_kfinger_free(run_job(ctx, oracle, seqs, plain, [setf]))
        L.fpm_kfinger_free(run_job(ctx, oracle, seqs, plain, [setf, ("fpm_kfinger_set_comb", (0,), OK)]))
        L.fpm_kfinger_free(run_job(ctx, oracle, seqs, plain, [("fpm_kfinger_set_comb", (1,), OK), setf,
                                                              ("fpm_kfinger_set_comb", (0,), OK)]))
        # on > 1 is refused and leaves the job as it was: combined; so is a fourth kind; after
        # the run the call is refused and the job fetches
        job = run_job(ctx, oracle, seqs, comb, [setf, ("fpm_kfinger_set_comb", (1,), OK),
                                                ("fpm_kfinger_set_comb", (2,), EINVAL),
                                                ("fpm_kfinger_set_comb", (0xFFFFFFFF,), EINVAL),
                                                ("fpm_kfinger_set_factorization", (3, 10), EINVAL)])
        try:
            assert L.fpm_kfinger_set_comb(job, 0) == EINVAL
            assert L.fpm_kfinger_set_comb(job, 1) == EINVAL
            h, nv = fetch(job, len(comb.lines))
            assert np.array_equal(nv, comb.n_vals)
        finally:
            L.fpm_kfinger_free(job)
    assert L.fpm_kfinger_set_comb(None, 1) == EINVAL
    assert L.fpm_kfinger_set_comb(None, 0) == EINVAL


def test_binding_refuses_unknown_names(ctx):
    for name in ("FOO", "CFL_COMB-10", "ICFL_COMB-3", "CFL_ICFL_COMB-0", "CFL_ICFL_COMB-",
                 "CFL_ICFL_COMB-%d" % (KMAX + 1)):
        with pytest.raises(ValueError):
            ctx.kfinger([b"ACGT"], factorization=name)


# ---- over stale memory ----------------------------------------------------------------------

@pytest.fixture(scope="module", params=(0x00, 0x5A, 0xFF), ids=["0x00", "0x5A", "0xFF"])
def pctx(request):
    """a context of this module's own with poison on (the shared `ctx` is left alone)"""
    c = fpmash.Context(0)
    c.set_poison(request.param)
    yield c
    c.close()


_models = {}


def _case(fact, w, seqs_of):
    key = (fact, w, seqs_of.__name__)
    if key not in _models:
        seqs = seqs_of(w)
        ids = K.default_ids(len(seqs))
        _models[key] = (seqs, K.Model(seqs, ids, w, fact, fast=True))
    return _models[key]


def _case_a(w):
    return F.window_seqs(w, R)[:7]


def _case_b(w):
    return [F.rand(900 + i, n) for i, n in enumerate([w + 50, 3, R + w + 9, w - 1])]


@pytest.mark.parametrize("fact", K.FACTS)
@pytest.mark.parametrize("wide", [False, True], ids=["lds", "wide"])
def test_over_poisoned_memory(pctx, oracle, fact, wide):
    """A, poison, a differently shaped B, poison, A again: the cut bits and the ICFL memory are
    written before they are read, in LDS and in the pooled regions"""
    wa = K.lds_window(fact) + 1 if wide else 100
    wb = K.lds_window(fact) + 30 if wide else 61
    sa, ma = _case(fact, wa, _case_a)
    sb, mb = _case(fact, wb, _case_b)
    check(pctx, oracle, sa, wa, fact, model=ma)
    pctx.poison_now()
    check(pctx, oracle, sb, wb, fact, model=mb)
    pctx.poison_now()
    check(pctx, oracle, sa, wa, fact, model=ma)
