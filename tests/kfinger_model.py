"""A thin model of `fpmash kfinger` and the fpm_kfinger_* calls, for the tests.

Lines come from fpmash.datagen.cfl_lines (pinned byte for byte to the fork's DNA1-CFL.txt),
hashes from oracle.get_hash_fp, References from oracle.fp_references over the model's text.
The two rules the generator adds are here: which ID a record's lines carry, and how many lines a
record makes.

cfl_lines costs about n x w interpreted steps for a record; the few wide-window cases (more
than FAST_STEPS of them in a record) take their lines from bin/cflgen instead, the C++
restatement that tests/test_cli.py pins to cfl_lines, and tests/test_kfinger_model.py checks the
two against each other through this module.
"""
import os
import subprocess

import numpy as np

from conftest import ROOT
from fpmash import datagen

CFLGEN = os.path.join(ROOT, "fp-mash_amd", "bin", "cflgen")
FAST_STEPS = 200_000


def line_id(header: bytes) -> bytes:
    """The ID of a record's lines from its header line (after '>' / '@', without the newline):
    kseq's name is the bytes up to the first whitespace byte and its comment the rest; the ID
    is the comment's first whitespace-separated token (lyn2vec's s_list[1]), or the name when
    there is none; lyn2vec then appends "_0"."""
    ws = b" \t\n\v\f\r"
    i = 0
    while i < len(header) and header[i] not in ws:
        i += 1
    name, comment = header[:i], header[i + 1:]
    tok = comment.split()
    return (tok[0] if tok else name) + b"_0"


def n_lines(n: int, w: int) -> int:
    """lines of a record of n bases at window w: none when empty, one when shorter than the
    window, else one per cyclic window start"""
    if n == 0:
        return 0
    return 1 if n < w else n


def _lines_fast(seq: bytes, w: int):
    # cflgen reads "<id>\t<sequence>" lines and writes "G00000<id>_0 ..." lines: an empty id
    assert b"\n" not in seq and b"\t" not in seq
    out = subprocess.run([CFLGEN, str(w), "4"], input=b"\t" + seq + b"\n", stdout=subprocess.PIPE,
                         check=True).stdout
    lines = out.split(b"\n")[:-1]
    assert all(l.startswith(b"G00000_0") for l in lines)
    return [l[len(b"G00000_0"):] + b"\n" for l in lines]


def record_lines(seq: bytes, full_id: bytes, w: int, fast=None):
    """the text lines of one record (bytes each); full_id carries its "_0\""""
    assert full_id.endswith(b"_0")
    if len(seq) == 0:
        return []
    if fast is None:
        fast = n_lines(len(seq), w) * min(len(seq), w) > FAST_STEPS
    if fast:
        return [full_id + body for body in _lines_fast(seq, w)]
    gid = full_id[:-2].decode("latin-1")
    return [l.encode("latin-1") for l in datagen.cfl_lines(seq, gid, w)]


class Model:
    """text, per-line values and the record -> line map of records `seqs` with full IDs `ids`"""

    def __init__(self, seqs, ids, w, max_lines=None):
        self.lines = []
        self.rec_first_line = [0]
        for s, i in zip(seqs, ids):
            got = record_lines(bytes(s), i, w)
            assert len(got) == n_lines(len(s), w)
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
        self.flat = (np.concatenate(self.vals) if self.vals else np.zeros(0, np.uint64)).astype(np.uint16)
        self._hash = {}

    def hashes(self, oracle, seed, use64):
        key = (seed, use64)
        if key not in self._hash:
            self._hash[key] = np.array([oracle.get_hash_fp(v, seed, use64) for v in self.vals],
                                       np.uint64 if use64 else np.uint32)
        return self._hash[key]


def window2(seq: bytes, full_id: bytes):
    """Model([seq], [full_id], 2) of one record of two bytes or more, in closed form, for records
    of millions of bytes: line i is the window (s[i], s[(i + 1) mod n]) upper-cased, one Lyndon
    factor of 2 when its first byte is below its second, else two of 1.  -> dict: rising (bool
    per line), n_vals, val_off, vals (u16) and text."""
    s = np.frombuffer(seq, np.uint8)
    assert len(s) >= 2
    s = np.where((s >= 0x61) & (s <= 0x7A), s - 0x20, s).astype(np.uint8)
    rising = s < np.roll(s, -1)
    n_vals = np.where(rising, 1, 2).astype(np.uint32)
    val_off = np.zeros(len(s) + 1, np.uint64)
    val_off[1:] = np.cumsum(n_vals, dtype=np.uint64)
    vals = np.ones(int(val_off[-1]), np.uint16)
    vals[val_off[:-1][rising].astype(np.int64)] = 2
    # "<id> 2\n" or "<id> 1 1\n"
    idb = np.frombuffer(full_id, np.uint8)
    size = len(idb) + np.where(rising, 3, 5)
    at = np.zeros(len(s) + 1, np.int64)
    at[1:] = np.cumsum(size)
    text = np.full(int(at[-1]), ord(" "), np.uint8)
    for j, c in enumerate(idb):
        text[at[:-1] + j] = c
    body = at[:-1] + len(idb)
    text[body + 1] = np.where(rising, ord("2"), ord("1"))
    text[body[~rising] + 3] = ord("1")
    text[at[1:] - 1] = ord("\n")
    return {"rising": rising, "n_vals": n_vals, "val_off": val_off, "vals": vals,
            "text": text.tobytes()}


def references(oracle, text: bytes, seed=42):
    """the References `sketch -fp` makes of the text: (name, length, u32 hashes in line order)"""
    refs, _used, _last = oracle.fp_references(text, seed=seed)
    return refs
