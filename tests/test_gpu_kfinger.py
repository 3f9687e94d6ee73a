"""fpm_kfinger_* on the device against tests/kfinger_model.py: for every case the line hashes
(u32 and u64, seed 42 and another), the value counts, the record -> line map, the values and the
text equal the model's, exactly.  Inputs are a few KB; R is the run length (window starts per
workgroup) and KMAX the widest window, both from fpm_kfinger_limits."""
import numpy as np
import pytest

import fpmash
import kfinger_model as M

pytestmark = pytest.mark.gpu

KMAX, R = fpmash.kfinger_limits()
SEEDS = (42, 7)


def rand(seed, n, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


def default_ids(n):
    return [b"G%05d_0" % i for i in range(n)]


def check(ctx, oracle, seqs, w, ids=None, max_lines=None, model=None):
    ids = default_ids(len(seqs)) if ids is None else ids
    m = model or M.Model(seqs, ids, w, max_lines)
    for use64 in (False, True):
        for seed in SEEDS:
            r = ctx.kfinger(seqs, window=w, seed=seed, use64=use64, max_lines=max_lines, ids=ids,
                            values=True, text=True)
            assert r["n_lines"] == len(m.lines)
            assert np.array_equal(r["rec_first_line"], m.rec_first_line)
            assert np.array_equal(r["n_vals"], m.n_vals)
            assert np.array_equal(r["val_off"], m.val_off)
            assert np.array_equal(r["vals"], m.flat)
            assert r["text"] == m.text
            assert r["hash"].dtype == (np.uint64 if use64 else np.uint32)
            assert np.array_equal(r["hash"], m.hashes(oracle, seed, use64))
    return m


def length_pattern(w):
    return [1, 2, w - 1, w, w + 1, R - 1, R, R + 1, R + w - 1, R + w, 2 * R + 1]


@pytest.mark.parametrize("w", [100, 1, 2, 3, 16, 17, 255, 256, 1000, KMAX])
def test_lengths(ctx, oracle, w):
    """the cyclic wrap of the last w - 1 starts, runs crossing workgroups, the short-record path
    (w - 1 is an empty record at w = 1: it makes no line)"""
    seqs = [rand(1000 * w + i, n) for i, n in enumerate(length_pattern(w))]
    m = check(ctx, oracle, seqs, w)
    assert len(m.lines) == sum(M.n_lines(len(s), w) for s in seqs)


@pytest.mark.parametrize("w", [99, 100])
def test_factor_count_extremes(ctx, oracle, w):
    """w values per line down to one, both count parities (the 8-byte Murmur tail), and Duval's
    repeated-factor step"""
    n = 300
    seqs = [b"A" * n, b"A" + b"T" * (n - 1), b"ACGT" * 75, b"TGCA" * 75, b"AT" * 149 + b"A",
            b"AAT" * 99 + b"AA",
            b"AT", b"TA", b"TCA"]             # short records: exactly 1, 2 and 3 values
    m = check(ctx, oracle, seqs, w)
    first = m.rec_first_line
    assert set(m.n_vals[int(first[0]):int(first[1])]) == {w}
    assert [int(m.n_vals[int(first[k])]) for k in (6, 7, 8)] == [1, 2, 3]
    assert {int(v) & 1 for v in m.n_vals} == {0, 1}
    # of the cyclic windows of A T^(n-1), the one starting at the A is a single Lyndon word
    assert 1 in m.n_vals[int(first[1]):int(first[2])]


def test_case_rule_and_unsigned_order(ctx, oracle):
    """a-z fold to A-Z and nothing else does; bytes compare unsigned (0x80 and 0xFF above '{')"""
    special = b"ACGTacgtNn@[`{\x7f\x80\xff"
    seqs = [rand(5, 300, special), rand(6, 99, special), rand(7, 100, special),
            b"aAaA" * 30, b"\xff\x80\x7f{`[@zZaA" * 12, b"\x80a\x7f", b"a\x80A"]
    check(ctx, oracle, seqs, 100)


def test_digit_boundaries_and_id_lengths(ctx, oracle):
    """factor lengths 9 / 10, 99 / 100 and 999 / 1000 in the text, IDs of 1 and 40 bytes"""
    w = 1000
    seqs = [b"A" + b"T" * (n - 1) for n in (9, 10, 99, 100, 999, 1000)]
    ids = [b"x_0", b"y" * 40 + b"_0", b"x_0", b"y" * 40 + b"_0", b"x_0", b"y" * 40 + b"_0"]
    m = check(ctx, oracle, seqs, w, ids=ids)
    heads = [int(m.rec_first_line[k]) for k in range(6)]
    assert [m.vals[h].tolist() for h in heads] == [[9], [10], [99], [100], [999], [1000]]


def test_many_short_records_share_a_workgroup(ctx, oracle):
    rng = np.random.default_rng(11)
    seqs = [rand(100 + i, int(rng.integers(1, 4))) for i in range(300)]
    m = check(ctx, oracle, seqs, 100)
    assert len(m.lines) == 300
    # short records between long ones, and enough short bytes to overflow one stage
    seqs = [rand(1, 150)] + [rand(200 + i, 90) for i in range(60)] + [rand(2, 101), b"", b"AC"]
    check(ctx, oracle, seqs, 100)


def test_max_lines(ctx, oracle):
    seqs = [rand(21, 130), rand(22, 50), rand(23, R + 40), rand(24, 3)]
    total = sum(M.n_lines(len(s), 100) for s in seqs)
    assert total == 130 + 1 + R + 40 + 1
    for cap in (0, 70, 130, 131, 131 + R + 1, total, total + 5):
        m = check(ctx, oracle, seqs, 100, max_lines=cap)
        assert len(m.lines) == min(cap, total)


def test_stage_seq_equals_host_staged(ctx, oracle):
    """a FASTA image with wrapped lines parsed on the device; the take mask drops the first, a
    middle and the last record"""
    recs = [(b"T%d G%d rest" % (i, i), rand(30 + i, n))
            for i, n in enumerate([120, 7, R + 130, 100, 99, 2 * R + 1, 64])]
    recs[3] = (b"NoComment", recs[3][1])
    image = b"".join(b">" + h + b"\n" + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60))
                     for h, s in recs)
    take = [0, 1, 1, 0, 1, 1, 0]
    ids = [M.line_id(h) for h, _ in recs]
    assert ids[3] == b"NoComment_0" and ids[0] == b"G0_0"
    kept = [s if t else b"" for (_, s), t in zip(recs, take)]
    m = M.Model(kept, ids, 100)
    for use64 in (False, True):
        for seed in SEEDS:
            d = ctx.kfinger_fasta([image], take=take, window=100, seed=seed, use64=use64,
                                  values=True, text=True)
            h = ctx.kfinger(kept, window=100, seed=seed, use64=use64, ids=ids, values=True,
                            text=True)
            assert np.array_equal(d["records"]["seq_len"], [len(s) for _, s in recs])
            for key in ("rec_first_line", "n_vals", "hash", "val_off", "vals"):
                assert np.array_equal(d[key], h[key]), key
            assert d["text"] == h["text"] == m.text
            assert np.array_equal(d["hash"], m.hashes(oracle, seed, use64))
            assert np.array_equal(d["rec_first_line"], m.rec_first_line)
    # every record taken (take = NULL), with a cut inside a record
    full = M.Model([s for _, s in recs], ids, 100, max_lines=200)
    d = ctx.kfinger_fasta([image], window=100, max_lines=200, values=True, text=True)
    assert d["text"] == full.text and np.array_equal(d["vals"], full.flat)
    assert np.array_equal(d["hash"], full.hashes(oracle, 42, False))


def test_refusals(ctx):
    for w in (0, KMAX + 1):
        with pytest.raises(fpmash.FpmError) as e:
            ctx.kfinger([b"ACGT"], window=w)
        assert e.value.code == fpmash.FPM_EINVAL
    # no record, and records without a base: no line, empty outputs
    for seqs in ([], [b"", b""]):
        r = ctx.kfinger(seqs, ids=default_ids(len(seqs)), values=True, text=True)
        assert r["n_lines"] == 0 and r["text"] == b"" and len(r["vals"]) == 0
        assert r["rec_first_line"].tolist() == [0] * (len(seqs) + 1)
