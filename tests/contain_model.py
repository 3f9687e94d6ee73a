"""Model of `contain` (CommandContain.cpp:264-300, 368-412): the literal walk of one pair, its
order-free form for strictly ascending lists, and the output line.  Lists are sequences of
non-negative ints (or numpy unsigned arrays); compares are plain integer compares, which is the
reference's unsigned compare at either hash width."""
import math
import struct

import numpy as np


def literal(R, Q):
    """containSketches as written -> (common, j)"""
    R = [int(x) for x in R]
    Q = [int(x) for x in Q]
    lr, lq = len(R), len(Q)
    common = 0
    denom = min(lr, lq)
    i = j = 0
    steps = 0
    while steps < denom and i < lr:
        if R[i] < Q[j]:
            i += 1
            steps -= 1
        elif Q[j] < R[i]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        steps += 1
    return common, j


def closed_form(R, Q):
    """(common, j) of two strictly ascending lists without walking them"""
    lr, lq = len(R), len(Q)
    m = min(lr, lq)
    if m == 0:
        return 0, 0
    top = int(R[lr - 1])
    jf = min(m, sum(1 for q in Q if int(q) <= top))
    rs = {int(x) for x in R}
    return sum(1 for q in Q[:jf] if int(q) in rs), jf


def grid(refs, qrys, fn=literal):
    """query-major (common, steps) arrays of every pair, index q * n_ref + r"""
    co = np.zeros(len(refs) * len(qrys), np.uint32)
    st = np.zeros(len(refs) * len(qrys), np.uint32)
    for q, Q in enumerate(qrys):
        for r, R in enumerate(refs):
            co[q * len(refs) + r], st[q * len(refs) + r] = fn(R, Q)
    return co, st


def grid_ascending(refs, qrys):
    """grid() of strictly ascending numpy lists by the closed form, vectorised (for the large
    rows of the dispatch tests, where the pure-Python walk would take seconds)"""
    co = np.zeros(len(refs) * len(qrys), np.uint32)
    st = np.zeros(len(refs) * len(qrys), np.uint32)
    for q, Q in enumerate(qrys):
        Q = np.asarray(Q)
        for r, R in enumerate(refs):
            R = np.asarray(R)
            m = min(len(R), len(Q))
            if m == 0:
                continue
            jf = min(m, int(np.searchsorted(Q, R[-1], side="right")))
            st[q * len(refs) + r] = jf
            co[q * len(refs) + r] = np.intersect1d(Q[:jf], R, assume_unique=True).size
    return co, st


def threshold(e):
    """-e as writeOutput(ContainOutput *, float error) sees it: rounded to float"""
    return struct.unpack("<f", struct.pack("<f", float(e)))[0]


def line(common, j, ref_name, qry_name, e=0.05):
    """the output line of one pair, or None when its error bound is above the threshold"""
    if j == 0:
        return None                       # error = inf
    error = 1.0 / math.sqrt(j)
    if not error <= threshold(e):
        return None
    return "%g\t%g\t%s\t%s" % (common / j, error, ref_name, qry_name)


def lines(refs, qrys, ref_names, qry_names, e=0.05):
    """the text `contain` prints: query-major, the reference index inner"""
    out = []
    for Q, qn in zip(qrys, qry_names):
        for R, rn in zip(refs, ref_names):
            c, j = literal(R, Q)
            s = line(c, j, rn, qn, e)
            if s is not None:
                out.append(s + "\n")
    return "".join(out)
