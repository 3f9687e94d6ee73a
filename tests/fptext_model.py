"""A plain-Python restatement of where the -fp text path (csrc/fingerprint.hip, the -fp half of
csrc/fpm_text_api.cpp) changes behaviour, and the inputs built to sit on those places.

The rules restated: lines are text.split(b"\\n") (a last line without '\\n' counts); the
newline index works in chunks of TEXT_CHUNK bytes and its chunk counts are scanned SCAN_BLOCK
to a scan block; fp_line_kernel gives a wave the 64 lines from l0 and stages the bytes from
line_start[max(l0 - 1, 0)] & ~15 to the end of line min(l0 + 63, n - 1) in LDS when they are
at most SPAN, else reads global memory; heads (line 0 and every line whose ID differs from the
one before) are counted HEAD_LINES lines to a workgroup; a Reference's length is its first
line's value count plus every line's; fpm_fp_text_refs fetches through the pinned ring when
n_refs <= RING_REFS.  tests/test_fptext_model.py shows on the CPU that each generated text
sits where its name says; tests/test_gpu_fptext_edges.py runs them on the device."""
import functools

import numpy as np

TEXT_CHUNK = 4096            # fpmash.fp_text_limits()[0]
SPAN = 4096                  # fpmash.fp_text_limits()[1]
HEAD_LINES = 1024            # fpmash.fp_text_limits()[2]
SCAN_BLOCK = 1024            # elements one scan workgroup takes (launch_exscan)
RING_REFS = (8 << 20) // 28  # References the pinned ring holds: 299,593
WAVE = 64
SPACES = b" \t\n\v\f\r"


# ---- the rules ------------------------------------------------------------------------

def lines_of(text):
    """the lines getline gives: split on '\\n', a last line without '\\n' counts"""
    parts = text.split(b"\n")
    return parts[:-1] if parts[-1] == b"" else parts


def line_starts(text):
    """line_start[0 .. n_nl]: 0, then 1 + the position of every '\\n' (the device index)"""
    buf = np.frombuffer(text, np.uint8)
    return np.concatenate([[0], np.flatnonzero(buf == 10) + 1]).astype(np.int64)


def n_lines_of(text, max_lines=None):
    n = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return n if max_lines is None else min(n, max_lines)


def wave_spans(text, max_lines=None):
    """[(s0, s1)] of every wave of fp_line_kernel over the text's first max_lines lines"""
    st = line_starts(text)
    n_nl, n = len(st) - 1, n_lines_of(text, max_lines)
    out = []
    for l0 in range(0, n, WAVE):
        s0 = int(st[max(l0 - 1, 0)]) & ~15
        ll = min(l0 + WAVE - 1, n - 1)
        s1 = int(st[ll + 1]) if ll < n_nl else len(text)
        out.append((s0, s1))
    return out


def span_bytes(text, max_lines=None):
    return [s1 - s0 for s0, s1 in wave_spans(text, max_lines)]


def staged(text, max_lines=None):
    """per wave: True where the span is staged in LDS, False where the wave reads global"""
    return [b <= SPAN for b in span_bytes(text, max_lines)]


def heads(ids):
    """first lines of the References: line 0 and every line whose ID differs from the last"""
    return [i for i in range(len(ids)) if i == 0 or ids[i] != ids[i - 1]]


def ref_lengths(hd, n_vals):
    """a Reference's length: its first line's value count, plus every line's"""
    n_vals = np.asarray(n_vals, np.int64)
    ends = list(hd[1:]) + [len(n_vals)]
    return [int(n_vals[a]) + int(n_vals[a:b].sum()) for a, b in zip(hd, ends)]


def chunks(text):
    return (len(text) + TEXT_CHUNK - 1) // TEXT_CHUNK


def scan_blocks(n):
    return (n + SCAN_BLOCK - 1) // SCAN_BLOCK


def head_groups(n_lines):
    return (n_lines + HEAD_LINES - 1) // HEAD_LINES


def join(lines, last_newline=True):
    return b"\n".join(lines) + (b"\n" if last_newline and lines else b"")


# ---- newline index --------------------------------------------------------------------

NL_LENGTHS = list(range(1, 81)) + [4095, 4096, 4097, 8191, 8192, 8193]


def nl_length_texts():
    """{(len, kind): text}: all '\\n'; x filler ending in '\\n'; the same without it"""
    out = {}
    for n in NL_LENGTHS:
        out[n, "all"] = b"\n" * n
        out[n, "last"] = b"x" * (n - 1) + b"\n"
        out[n, "none"] = b"x" * n
    return out


NL_POSITIONS = list(range(64)) + [4095, 4096, 4097]


def nl_position_texts():
    """{p: a 4,200-byte filler text whose only '\\n' is byte p}"""
    return {p: b"x" * p + b"\n" + b"x" * (4200 - p - 1) for p in NL_POSITIONS}


def nl_full_chunk():
    """8,197 '\\n': every thread of the first two chunks counts 16"""
    return b"\n" * 8197


STALE_LENGTHS = (1, 2, 3, 17, 4097)


@functools.lru_cache(maxsize=None)
def two_scan_blocks_text():
    """1025 * 4096 + 7 bytes of 40..79-byte lines from 53 distinct line bodies: 1,026 chunk
    counts, more than the 1,024 a scan block takes; the last line has no '\\n'"""
    rng = np.random.default_rng(77)
    bodies = []
    for i in range(53):
        vals = b" ".join(b"%d" % v for v in rng.integers(0, 1 << 40, 1 + i % 3))
        body = b"read%02d" % (i % 11) + b"_" * (i % 7) + b" " + vals
        bodies.append(body.ljust(40 + (i * 3) % 40))             # trailing blanks
    want = 1025 * TEXT_CHUNK + 7
    picks = rng.integers(0, len(bodies), want // 40 + 1)
    out, size = [], 0
    for p in picks:
        ln = bodies[int(p)]
        if size + len(ln) + 1 > want - 90:
            break
        out.append(ln)
        size += len(ln) + 1
    # the rest as one last line of filler digits behind an ID, without '\n'
    tail = b"tail " + b"7" * (want - size - 5)
    return join(out) + tail


# ---- line kernel spans ----------------------------------------------------------------

def short_line(i):
    """a short -fp line with 0..5 values, its ID changing every few lines"""
    return b"k%d" % (i // 3) + b"".join(b" %d" % (i * 7919 + j * 104729) for j in range(i % 6))


def span_text(span, residue, n_lines=128):
    """n_lines short lines where wave 1 (lines 64..127, and line 63 before them) has a span of
    exactly `span` bytes and line 63 starts at `residue` modulo 16"""
    lines = [short_line(i) for i in range(n_lines)]
    start63 = sum(len(x) + 1 for x in lines[:63])
    lines[62] += b" " * ((residue - start63) % 16)              # trailing blanks move line 63
    have = sum(len(x) + 1 for x in lines[63:128]) + residue
    assert have < span
    lines[100] = b"I" * (span - have) + lines[100]               # a long ID makes up the rest
    return join(lines)


def long_previous_line_text():
    """128 lines: line 63 is 5,000 bytes, lines 64..127 are short, so wave 1 reads global
    memory only because of the line before it"""
    lines = [short_line(i) for i in range(128)]
    lines[63] = b"k21 " + b" ".join(b"%d" % (i * 31) for i in range(2000))[:4996]
    assert len(lines[63]) == 5000
    return join(lines)


def long_middle_line_text():
    """70 lines with one of 5,000 bytes at line 30, among short ones"""
    lines = [short_line(i) for i in range(70)]
    lines[30] = b"k10 " + b"18446744073709551615 " * 237 + b"1" * 19
    assert len(lines[30]) == 5000
    return join(lines)


LINE_COUNTS = (1, 63, 64, 65, 255, 256, 257)


def counted_text(n, last_newline=True):
    return join([short_line(i) for i in range(n)], last_newline)


def block_first_id_texts():
    """300 lines, IDs changing every 32 lines: at lines 64 and 256 ('differs'), or five lines
    before them ('equal')"""
    def text(shift):
        return join([b"g%d %d %d" % ((i + shift) // 32, i, i * i) for i in range(300)])
    return {"differs": text(0), "equal": text(5)}


def id_pair_text():
    """adjacent IDs of equal length differing in the last byte only, and IDs that are a prefix
    of their neighbour, for ID lengths 1..9 (inside a word, on its edge, over two words)"""
    lines = []
    for n in range(1, 10):
        stem = b"ABCDEFGHI"[:n - 1]
        lines += [stem + b"x 1", stem + b"y 2", stem + b"y 3"]
        if n > 1:
            lines += [stem + b" 4", stem + b"y 5", stem + b"yz 6", stem + b"y 7"]
    return join(lines)


def id_residue_text():
    """IDs behind 0..7 leading blanks and tabs: every start residue modulo 4, for a line and
    for the line before it"""
    lines = []
    for i in range(48):
        lead = (b" \t" * 4)[:(i * 5) % 8]
        lines.append(lead + b"id%d %d" % (i // 2, i))
    return join(lines)


# ---- value grammar --------------------------------------------------------------------

GRAMMAR = (
    [("u64 max - 5 + %d" % i, b"v 1 1844674407370955161%d 2" % i) for i in range(10)] +
    [("twenty nines", b"v 1 99999999999999999999 2"),
     ("thirty zeros then 7", b"v " + b"0" * 30 + b"7 2"),
     ("minus zero", b"v -0 2"),
     ("minus one", b"v -1 2"),
     ("minus u64 max", b"v -18446744073709551615 2"),
     ("minus 2^64", b"v 1 -18446744073709551616 2"),
     ("plus alone", b"v 1 + 2"),
     ("minus alone", b"v 1 - 2"),
     ("plus minus", b"v 1 +-1 2"),
     ("minus blank", b"v 1 - 1"),
     ("one plus two", b"v 1+2 3"),
     ("one minus two", b"v 1-2 3"),
     ("digits then letters", b"v 12abc 4"),
     ("hex", b"v 0x1f 4"),
     ("point", b"v 1.5 4"),
     ("exponent", b"v 1e5 4"),
     ("NUL between numbers", b"v 1\x002"),
     ("NUL token between numbers", b"v 1 \x00 2"),
     ("vertical tab", b"v\v1\v2"),
     ("form feed", b"v\f1\f2"),
     ("carriage return", b"v\r1\r2\r")] +
    [("%d values" % n, b"v" + b"".join(b" %d" % (1000 + j) for j in range(n)))
     for n in (0, 1, 2, 3, 15, 16, 17)] +
    [("ID then blanks", b"v  \t "),
     ("blank line", b" \t  "),
     ("lone carriage return", b"\r")]
)


def grammar_text(long_line=False):
    """the GRAMMAR lines in one wave; long_line: with a 5,000-byte line among them, so the wave
    reads global memory"""
    lines = [g for _n, g in GRAMMAR]
    assert len(lines) < WAVE - 1
    if long_line:
        lines.insert(20, b"v " + b"12345678 " * 555 + b"123")
        assert len(lines[20]) == 5000
    return join(lines)


# ---- heads and References -------------------------------------------------------------

HEAD_COUNTS = (1023, 1024, 1025, 2049)
HEAD_AT = (0, 7, 8, 1023, 1024, 1025, 2047, 2048)      # 4t + 3 / 4t + 4: a thread's last / first


def head_text(n):
    """n lines whose IDs change at the lines of HEAD_AT below n (and nowhere else)"""
    hd = [h for h in HEAD_AT if h < n]
    lines = [b"r%d" % sum(1 for h in hd if h <= i) + b" %d" % i * (i % 4) for i in range(n)]
    return join(lines), hd


def all_heads_text(n=1025):
    return join([b"i%d %d" % (i, i) for i in range(n)])


ONE_REF_LINES = (64, 65, 129, 1025)


def one_ref_text(n):
    return join([b"only" + b" %d" % i * (i % 5) for i in range(n)])


def n_refs_text(n_refs):
    return join([b"ref%d %d %d" % (r, r, j) for r in range(n_refs) for j in range(1 + r % 3)])


def doubled_first_text():
    """first lines of 3, 0 and 1 values: lengths 3 + (3 + 2), 0 + (0 + 4), 1 + 1"""
    return join([b"a 1 2 3", b"a 4 5", b"b", b"b 1 2 3 4", b"c 9"])


def alternating_text(n):
    """n lines 'a' / 'b' in turn, no values: every line a Reference"""
    return (b"a\nb\n" * ((n + 1) // 2))[:2 * n]


RING_EDGE = (RING_REFS, RING_REFS + 1)
TWO_HEAD_SCAN_LINES = SCAN_BLOCK * HEAD_LINES + 1 + HEAD_LINES     # 1,049,601


# ---- random strings for the parse pin ---------------------------------------------------

TOKENS = [b"+", b"-", b"18446744073709551615", b"18446744073709551616", b"0" * 26, b"0x1f",
          b".", b"e", b"\x00", b" ", b"\t", b"\n", b"\v", b"\f", b"\r", b"1", b"7", b"42",
          b"id", b"a", b"9", b"99999999999999999999", b"18446744073709551614", b"12abc", b"0",
          b"5"]


def random_strings(seed, n):
    """n strings of 1..12 TOKENS each, abutting; every second one behind an ID and a blank"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 13, n)
    picks = rng.integers(0, len(TOKENS), int(counts.sum()))
    out, at = [], 0
    for i, c in enumerate(counts):
        s = b"".join(TOKENS[int(t)] for t in picks[at:at + c])
        out.append(b"id " + s if i & 1 else s)
        at += c
    return out


def small_texts():
    """{name: text} of every generated text under 1 MB (the parse pin runs over all of them)"""
    out = {}
    for (n, kind), t in nl_length_texts().items():
        out["nl %d %s" % (n, kind)] = t
    for p, t in nl_position_texts().items():
        out["nl at %d" % p] = t
    out["nl full chunk"] = nl_full_chunk()
    for span in (SPAN, SPAN + 1):
        for res in (0, 15):
            out["span %d residue %d" % (span, res)] = span_text(span, res)
    out["long previous line"] = long_previous_line_text()
    out["long middle line"] = long_middle_line_text()
    for n in LINE_COUNTS:
        out["%d lines" % n] = counted_text(n)
    out["65 lines, no last newline"] = counted_text(65, last_newline=False)
    out["200 lines"] = counted_text(200)
    for k, t in block_first_id_texts().items():
        out["block first ID " + k] = t
    out["ID pairs"] = id_pair_text()
    out["ID residues"] = id_residue_text()
    out["grammar"] = grammar_text()
    out["grammar, global"] = grammar_text(long_line=True)
    for n in HEAD_COUNTS:
        out["heads %d" % n] = head_text(n)[0]
    out["all heads"] = all_heads_text()
    for n in ONE_REF_LINES:
        out["one Reference of %d" % n] = one_ref_text(n)
    for n in (1, 3, 4, 5):
        out["%d References" % n] = n_refs_text(n)
    out["doubled first"] = doubled_first_text()
    for n in RING_EDGE:
        out["%d References" % n] = alternating_text(n)
    assert all(len(t) < 1_000_000 for t in out.values())
    return out
