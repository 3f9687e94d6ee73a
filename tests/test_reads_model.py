"""Pins tests/reads_model.py, the reads-mode checker (MinHashHeap::tryInsert with
multiplicityMinimum = m, MinHashHeap.cpp:68-146), on the CPU:
  m = 1   it is the oracle's literal heap (oracle.sketch_batch(counts=True), itself pinned to the
          reference's reads.msh by tests/test_oracle_golden.py);
  m >= 2  its hashes are the first s of the hashes seen >= m times, its counts their full
          counts (an oracle sketch wider than the window count) except the maximum of a full
          sketch, which follows the closed form with T, whatever the record order;
  the set-size formula gives the length stored in reads.msh.
"""
import numpy as np
import pytest

import mshfmt
import reads_model as RM
from conftest import GOLDEN


def one_group(oracle, recs, k, s):
    h, c = oracle.sketch_batch(oracle.params(k=k, s=s), recs, groups=[0] * len(recs), n_groups=1,
                               counts=True)
    return h[0], c[0]


@pytest.fixture(scope="module")
def base():
    return RM.base_reads()


@pytest.fixture(scope="module")
def streams(oracle, base):
    return {k: RM.window_hashes(oracle, base, k) for k in (21, 12)}


@pytest.mark.parametrize("k,s", [(21, 50), (21, 1), (12, 100), (21, 1000), (21, 100000)])
def test_m1_is_the_oracle_heap(oracle, base, streams, k, s):
    h, c = RM.model_sketch(streams[k], s, 1)
    eh, ec = one_group(oracle, base, k, s)
    assert np.array_equal(h, eh)
    assert np.array_equal(c, ec)


@pytest.mark.parametrize("k,s,m", [(21, 50, 2), (21, 1, 2), (12, 100, 3), (21, 1000, 2),
                                   (21, 50, 4)])
def test_min_copies_hashes_and_counts(oracle, base, streams, k, s, m):
    stream = streams[k]
    ah, ac = one_group(oracle, base, k, len(stream) + 1)     # every distinct hash, full counts
    keep = ac >= m
    fh, fc = ah[keep][:s], ac[keep][:s]
    h, c = RM.model_sketch(stream, s, m)
    assert np.array_equal(h, fh)
    full = len(fh) == s
    n = len(fh) - 1 if full else len(fh)
    assert np.array_equal(c[:n], fc[:n])
    ch, cc = RM.closed_form(stream, s, m)
    assert np.array_equal(h, ch)
    assert np.array_equal(c, cc)
    if full:
        assert m <= c[-1] <= fc[-1]


def test_maximum_count_follows_record_order(oracle):
    """`unit * 30` between / after two copies of a record y: the same hashes, the maximum's
    count differs (s puts a unit hash on top with y hashes below it: with y's second copy last
    the heap settles at the end of the stream, so the maximum counts all 30 of its occurrences;
    with both copies first it settles inside unit's second copy), and both equal the closed
    form."""
    orders, s = RM.order_inputs(oracle)
    got = []
    for order in orders:
        stream = RM.window_hashes(oracle, order, 21)
        for ss, m in ((s, 2), (s, 3), (s + 7, 2), (5, 2)):
            h, c = RM.model_sketch(stream, ss, m)
            ch, cc = RM.closed_form(stream, ss, m)
            assert np.array_equal(h, ch)
            assert np.array_equal(c, cc)
        got.append(RM.model_sketch(stream, s, 2))
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1][:-1], got[1][1][:-1])
    assert got[0][1][-1] == 30 and got[1][1][-1] == 2


def test_set_size_formula_on_fixture():
    ref = mshfmt.read_msh(f"{GOLDEN}/reads.msh")["references"][0]
    assert ref["length"] == 502359
    assert RM.set_size(ref["hashes64"], use64=True) == 502359
    assert RM.set_size([], use64=True) == 0
    assert RM.set_size([1 << 31, 1 << 30], use64=False) == 4
