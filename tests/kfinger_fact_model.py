"""tests/kfinger_model.py with a factorization: the model of `fpmash kfinger -F` and of
fpm_kfinger_set_factorization, for the tests.

Lines come from fpmash.datagen.cfl_lines(..., factorization=...), whose ICFL and CFL_ICFL-T are
pinned to lyn2vec's own results (tests/golden/icfl_words.json.gz, DNA1-ICFL.txt.gz,
DNA1-CFL_ICFL-10.txt.gz; tests/golden/KFINGER.md) by tests/test_kfinger_fact_model.py;
wide-window cases take them from bin/cflgen's third argument, which the same file pins to the Python restatement.

The inputs the GPU tests run are built here, so that the CPU tests can show, from the counters
the restatement returns (steps, merges, the longest border chain, the largest `last`), that each
one sits on the edge it is named for.
"""
import gzip
import os
import subprocess

import numpy as np

from conftest import GOLDEN
import kfinger_model as M
from fpmash import datagen

# ICFL, lyn2vec's three CFL_ICFL thresholds, and the smallest threshold there is
FACTS = ("ICFL", "CFL_ICFL-10", "CFL_ICFL-20", "CFL_ICFL-30", "CFL_ICFL-1")


def golden(name):
    """the bytes of the gzipped fixture tests/golden/<name>.gz"""
    with gzip.open(os.path.join(GOLDEN, name + ".gz"), "rb") as f:
        return f.read()


def rand(seed, n, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


def default_ids(n):
    return [b"G%05d_0" % i for i in range(n)]


def _lines_fast(seq: bytes, w: int, fact: str):
    assert b"\n" not in seq and b"\t" not in seq
    out = subprocess.run([M.CFLGEN, str(w), "4", fact], input=b"\t" + seq + b"\n",
                         stdout=subprocess.PIPE, check=True).stdout
    lines = out.split(b"\n")[:-1]
    assert all(l.startswith(b"G00000_0") for l in lines)
    return [l[len(b"G00000_0"):] + b"\n" for l in lines]


def record_lines(seq: bytes, full_id: bytes, w: int, fact: str, fast=None):
    """kfinger_model.record_lines under factorization `fact`"""
    assert full_id.endswith(b"_0")
    if len(seq) == 0:
        return []
    if fast is None:
        fast = M.n_lines(len(seq), w) * min(len(seq), w) > M.FAST_STEPS // 4
    if fast:
        return [full_id + body for body in _lines_fast(seq, w, fact)]
    gid = full_id[:-2].decode("latin-1")
    return [l.encode("latin-1") for l in datagen.cfl_lines(seq, gid, w, factorization=fact)]


def batch_lines(seqs, ids, w: int, fact: str):
    """record_lines(..., fast=True) of every record, from one run of cflgen over all of them
    (a process per record costs more than its lines once there are a thousand records)"""
    assert all(i.endswith(b"_0") for i in ids)
    assert not any(b"\n" in s or b"\t" in s for s in seqs)
    out = subprocess.run([M.CFLGEN, str(w), "4", fact], stdout=subprocess.PIPE, check=True,
                         input=b"".join(b"\t" + bytes(s) + b"\n" for s in seqs if len(s))).stdout
    bodies = out.split(b"\n")[:-1]
    assert all(l.startswith(b"G00000_0") for l in bodies)
    res, at = [], 0
    for s, i in zip(seqs, ids):
        n = M.n_lines(len(s), w)
        res.append([i + l[len(b"G00000_0"):] + b"\n" for l in bodies[at:at + n]])
        at += n
    assert at == len(bodies)
    return res


class Model(M.Model):
    """kfinger_model.Model under factorization `fact`"""

    def __init__(self, seqs, ids, w, fact, max_lines=None, fast=None):
        self.lines = []
        self.rec_first_line = [0]
        batch = batch_lines(seqs, ids, w, fact) if fast else None
        for r, (s, i) in enumerate(zip(seqs, ids)):
            got = batch[r] if batch else record_lines(bytes(s), i, w, fact, fast)
            assert len(got) == M.n_lines(len(s), w)
            self.lines += got
            if max_lines is not None:
                del self.lines[max_lines:]
            self.rec_first_line.append(len(self.lines))
        self.rec_first_line = np.array(self.rec_first_line, np.uint64)
        self.text = b"".join(self.lines)
        self.vals = [np.array(l.split()[1:], dtype=np.uint64) for l in self.lines]
        self.n_vals = np.array([len(v) for v in self.vals], np.uint32)
        self.val_off = np.zeros(len(self.vals) + 1, np.uint64)
        self.val_off[1:] = np.cumsum(self.n_vals)
        self.flat = (np.concatenate(self.vals) if self.vals
                     else np.zeros(0, np.uint64)).astype(np.uint16)
        self._hash = {}


def cut(m, max_lines):
    """Model(..., max_lines=max_lines) from the uncut model m of the same records: its first
    max_lines lines"""
    c = object.__new__(Model)
    c.lines = m.lines[:max_lines]
    c.rec_first_line = np.minimum(m.rec_first_line, np.uint64(max_lines))
    c.text = b"".join(c.lines)
    c.vals = m.vals[:max_lines]
    c.n_vals = m.n_vals[:max_lines]
    c.val_off = m.val_off[:len(c.lines) + 1]
    c.flat = m.flat[:int(c.val_off[-1])]
    c._hash = {}
    c.hashes = lambda oracle, seed, use64: m.hashes(oracle, seed, use64)[:max_lines]
    return c


def windows(seq: bytes, w: int):
    """the upper-cased windows of one record, in line order"""
    s = seq.upper()
    if not s:
        return []
    if len(s) < w:
        return [s]
    ss = s + s[:w]
    return [ss[i:i + w] for i in range(len(s))]


def counters(seqs, w, fact="ICFL", every=1):
    """What the restatement counts over the lines of `seqs` (over every `every`-th line, where
    all of them would take too long): per line its steps, glued pieces (merges), longest border
    chain in links and largest `last`; -> the maxima of the four and the number of lines with a
    merge and with last > 0."""
    out = {"steps": 0, "merges": 0, "chain": 0, "last": 0, "lines_merging": 0, "lines_last": 0,
           "lines": 0}
    for s in seqs:
        for win in windows(bytes(s), w)[::every]:
            st = {}
            datagen.factor_lengths(win, fact, st)
            out["lines"] += 1
            for k in ("steps", "merges", "chain", "last"):
                out[k] = max(out[k], st.get(k, 0))
            out["lines_merging"] += st.get("merges", 0) > 0
            out["lines_last"] += st.get("last", 0) > 0
    return out


# ---- the inputs of tests/test_gpu_kfinger_fact.py ------------------------------------------

def length_pattern(w, R):
    return [1, 2, w - 1, w, w + 1, R - 1, R, R + 1, R + w, 2 * R + 1]


def window_seqs(w, R):
    """random DNA at the record lengths around the window and the run length"""
    return [rand(7000 * w + i, n) for i, n in enumerate(length_pattern(w, R))]


def wide_seqs(w, R):
    return [rand(9000 + i, n) for i, n in enumerate([w - 1, w, w + 1, R + w])]


def max_lines_seqs(R):
    """a long record, a short one, a record of more than one run, a short one"""
    return [rand(21, 130), rand(22, 50), rand(23, R + 40), rand(24, 3)]


def short_record_sets():
    """300 records of 1 to 11 bytes (packs of up to 256 share a workgroup); then short records
    between long ones, with enough short bytes to overflow one stage"""
    rng = np.random.default_rng(11)
    many = [rand(100 + i, int(rng.integers(1, 12)), b"AC") for i in range(300)]
    mixed = [rand(1, 150)] + [rand(200 + i, 90) for i in range(60)] + [rand(2, 101), b"", b"AC"]
    return many, mixed


def stage_seq_records(R):
    """(header, sequence) records of a FASTA image and the take mask over them"""
    recs = [(b"T%d G%d rest" % (i, i), rand(30 + i, n)) for i, n in enumerate([120, 7, R + 130, 99])]
    return recs, [1, 0, 1, 1]


def plan_descs(lens, w, R, stage, max_lines=None):
    """the descriptors fpm_kfinger_stage makes of records of these lengths (one per workgroup
    of a narrow window; a wide window's workgroups share them out): a record of w bytes or more
    gives one per R window starts; records shorter than w, one line each, share one while they
    follow each other, number at most R and fill at most `stage` bytes.  max_lines ends the job
    inside a record or before one.  fpm_kfinger_wide_groups of a job with fewer descriptors
    than the device takes workgroups is this number (tests/test_gpu_kfinger_scale.py)."""
    descs = line = pack_n = pack_bytes = 0
    cap = float("inf") if max_lines is None else max_lines
    for n in lens:
        if n == 0 or line >= cap:
            continue
        if n < w:
            if pack_n == R or pack_bytes + n > stage:
                pack_n = pack_bytes = 0
            descs += pack_n == 0
            pack_n += 1
            pack_bytes += n
            line += 1
            continue
        pack_n = pack_bytes = 0
        lines = min(n, cap - line)
        descs += -(-lines // R)
        line += lines
    return descs


def stride_lens(n_desc, w, R):
    """record lengths that make exactly n_desc cheap descriptors of both kinds: a record
    shorter than the window (one line, a pack of its own between two long records) alternates
    with one of w .. w + 7 bytes (one descriptor of that many lines), and every 50th record has
    2 R + 5 bytes: three descriptors, the last one of five lines"""
    assert w + 7 <= R
    lens, descs = [], 0
    while descs < n_desc:
        i = len(lens)
        if i % 2 == 0:
            lens.append(1 + (i // 2 * 37) % (w - 1))
        elif i % 50 == 49 and descs + 3 <= n_desc:
            lens.append(2 * R + 5)
        else:
            lens.append(w + i // 2 % 8)
        descs += -(-lens[-1] // R) if lens[-1] >= w else 1
    return lens


def stride_seqs(n_desc, w, R):
    return [rand(31000 + i, n) for i, n in enumerate(stride_lens(n_desc, w, R))]


W = 100
# W distinct ascending bytes from 0x25 on that upper-casing leaves apart (no a-z): window 0 has
# W - 1 steps and W factors of 1
ASCENDING = bytes([c for c in range(0x25, 0x100) if not 0x61 <= c <= 0x7A][:W])
DESCENDING = ASCENDING[::-1]                        # window 0: no step, one factor
ONE_LETTER = b"A" * 130
# TTG-periodic text ending in a break above its letters: the scan runs over the whole period
# run, `last` is a long border and the chain walks a link per period
PERIODIC = b"TTG" * 33 + b"Z"
# TTTG leaves borders inside the period too
PERIODIC4 = b"TTTG" * 24 + b"TTTZ"
# short records with a piece glued onto the factor behind it (the merge branch).  CAACACC, the
# shortest there is over three letters: the step at 0 stops at CAACA|C with last = 2 (the border
# CA, followed by A < C), piece CAA; the step at 3 stops at CAC|C with last = 1, piece CA; CC is
# the last factor.  2 > 1 makes CA a factor; 2 > 2 fails, so CAA is glued onto it: 5 2.
MERGING = [b"CAACACC", b"GACGAGG", b"ACAACACC", b"CAACACC" * 9, b"TGGTGTT" + b"CAACACC"]
EXTREMES = [ASCENDING, DESCENDING, ONE_LETTER, b"ACGT" * 25, b"TGCA" * 25, PERIODIC, PERIODIC4] + \
    MERGING + [b"T", b"TA", b"AT", b"TCA", b"ACT"]


def threshold_seq(T):
    """a short record with the Lyndon factors A T^T (T + 1 bytes: split into 1, T) and A T^(T-1)
    (T bytes: kept)"""
    return b"A" + b"T" * T + b"A" + b"T" * (T - 1)


SPECIAL = b"ACGTacgtNn@[`{\x7f\x80\xff"


def byte_rule_seqs():
    """lowercase, bytes >= 0x80, and 0x24, which lyn2vec cannot take and the product factorizes
    like any other byte"""
    return [rand(5, 230, SPECIAL), rand(6, 99, SPECIAL), b"aAaA" * 30,
            b"\xff\x80\x7f{`[@zZaA" * 12, b"\x80a\x7f", b"GA$T", rand(8, 150, b"ACGT$"),
            b"$" * 5 + b"A$%$", rand(9, 60, b"$%#")]
