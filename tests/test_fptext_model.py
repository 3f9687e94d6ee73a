"""CPU tests behind tests/test_gpu_fptext_edges.py.

The expected side of every -fp text test is oracle.fp_parse, a C restatement of getline /
`ss >> id` / `while (ss >> v)` whose number reader is the expression the device kernel uses.
Here that restatement is held to libstdc++'s own istream (oracle/fp_istream.cpp) on random
strings of the tokens where the two could part (signs, 2^64 - 1, 2^64, long runs of zeros, hex,
'.', 'e', NUL, the six space bytes), on the named grammar lines, and on every generated text
under 1 MB.  The rest shows that the texts of tests/fptext_model.py sit on the edges they are
named for, by the model's restatement of the kernels' rules."""
import numpy as np
import pytest

import fptext_model as M

O = pytest.importorskip("oracle.oracle")


def assert_same_parse(text, **kw):
    a = O.fp_parse_arrays(text, **kw)
    b = O.fp_parse_arrays(text, istream=True, **kw)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y), text[:200]
    assert a[4] == b[4]
    return a


def test_parse_equals_istream_on_random_strings():
    """200,000 strings: each a text of its own for the first 4,000 (the end of the text met
    in every state), the rest 2,000 to a text, one per line ('\\n' is among the tokens, so a
    string may be several lines)"""
    strings = M.random_strings(2024, 200_000)
    assert len(strings) == 200_000 and len(M.TOKENS) == 26
    n_lines = n_vals = 0
    for s in strings[:4000]:
        assert_same_parse(s)
    for at in range(4000, len(strings), 2000):
        a = assert_same_parse(b"\n".join(strings[at:at + 2000]))
        n_lines += len(a[0])
        n_vals += len(a[2])
    assert n_lines >= 196_000 and n_vals > 50_000                # the value loop did run


def test_parse_equals_istream_on_grammar():
    for name, line in M.GRAMMAR:
        for text in (line, line + b"\n", b"w 5\n" + line + b"\nx 6"):
            assert_same_parse(text)
    assert len({n for n, _l in M.GRAMMAR}) == len(M.GRAMMAR) == 41
    # what the grammar lines are there to show, by the restatement now pinned
    vals = dict(zip((n for n, _l in M.GRAMMAR), O.fp_parse(M.grammar_text())[1]))
    top = 2 ** 64 - 1
    for i in range(10):
        assert list(vals["u64 max - 5 + %d" % i]) == ([1, top - 5 + i, 2] if i <= 5 else [1])
    assert list(vals["twenty nines"]) == [1]
    assert list(vals["thirty zeros then 7"]) == [7, 2]
    assert list(vals["minus zero"]) == [0, 2]
    assert list(vals["minus one"]) == [top, 2]
    assert list(vals["minus u64 max"]) == [1, 2]
    assert list(vals["minus 2^64"]) == [1]
    for n in ("plus alone", "minus alone", "plus minus", "minus blank"):
        assert list(vals[n]) == [1]
    assert list(vals["one plus two"]) == [1, 2, 3]
    assert list(vals["one minus two"]) == [1, top - 1, 3]
    assert list(vals["digits then letters"]) == [12]
    assert list(vals["hex"]) == [0] and list(vals["point"]) == [1]
    assert list(vals["exponent"]) == [1]
    assert list(vals["NUL between numbers"]) == [1]
    assert list(vals["NUL token between numbers"]) == [1]
    for n in ("vertical tab", "form feed", "carriage return"):
        assert list(vals[n]) == [1, 2]
    for n in (0, 1, 2, 3, 15, 16, 17):
        assert len(vals["%d values" % n]) == n
    ids = dict(zip((n for n, _l in M.GRAMMAR), O.fp_parse(M.grammar_text())[0]))
    assert ids["ID then blanks"] == b"v" and ids["blank line"] == b""
    assert ids["lone carriage return"] == b""


def test_parse_equals_istream_on_generated_texts():
    texts = M.small_texts()
    assert len(texts) > 300
    for name, t in texts.items():
        a = assert_same_parse(t)
        assert len(a[0]) == M.n_lines_of(t) == len(M.lines_of(t)), name
    for cap in (64, 65):
        assert assert_same_parse(M.counted_text(200), limit=cap)[4] == cap


def test_reference_parse_of_grammar(tmp_path):
    """the reference's own loop (istringstream parse, its compiled getHashFingerPrint) over the
    grammar texts as files: Reference count and hash checksum as oracle.fp_references gives"""
    if O.ref() is None:
        pytest.skip("oracle/_ref not built")
    for i, text in enumerate((M.grammar_text(), M.grammar_text(long_line=True))):
        path = tmp_path / ("g%d.txt" % i)
        path.write_bytes(text)
        refs, used, _last = O.fp_references(text)
        want_sum = sum(int(h.astype(np.uint64).sum()) for _n, _l, h in refs) % 2 ** 64
        got = O.ref_fp_sketch_files([str(path)])
        assert got == (len(refs), used, want_sum)
        assert used == len(M.lines_of(text))


# ---- the generators' promises -----------------------------------------------------------

def test_model_rules():
    assert M.lines_of(b"") == [] and M.lines_of(b"\n") == [b""]
    assert M.lines_of(b"a\n\nb") == [b"a", b"", b"b"] and M.n_lines_of(b"a\n\nb") == 3
    assert list(M.line_starts(b"a\n\nb")) == [0, 2, 3]
    assert M.heads([b"a", b"a", b"b", b"a"]) == [0, 2, 3]
    assert M.ref_lengths([0, 2], [3, 2, 0, 4]) == [3 + 5, 0 + 4]
    assert M.RING_REFS == 299_593 and (M.RING_REFS + 1) * 28 > 8 << 20 >= M.RING_REFS * 28
    # a wave's span starts at the 16-byte block of the line before it
    t = M.join([b"x" * 20] * 130)
    assert M.wave_spans(t)[:2] == [(0, 64 * 21), ((63 * 21) & ~15, 128 * 21)]
    assert M.wave_spans(t, max_lines=65)[1] == ((63 * 21) & ~15, 65 * 21)
    assert M.wave_spans(t[:-1])[2] == ((127 * 21) & ~15, len(t) - 1)


def test_newline_texts():
    texts = M.nl_length_texts()
    assert len(texts) == 3 * 86
    for (n, kind), t in texts.items():
        assert len(t) == n
        assert M.n_lines_of(t) == (n if kind == "all" else 1)
    assert {n % 4 for n in M.NL_LENGTHS} == {0, 1, 2, 3} and {n % 16 for n in M.NL_LENGTHS} == \
        set(range(16))
    for p, t in M.nl_position_texts().items():
        assert len(t) == 4200 and t.count(b"\n") == 1 and t[p] == 10
    full = M.nl_full_chunk()
    assert M.chunks(full) == 3 and full[:M.TEXT_CHUNK].count(b"\n") == M.TEXT_CHUNK
    big = M.two_scan_blocks_text()
    assert len(big) == 1025 * 4096 + 7 and M.chunks(big) == 1026
    assert M.scan_blocks(M.chunks(big)) == 2 and M.scan_blocks(1024) == 1
    lens = [len(x) for x in M.lines_of(big)[:-1]]
    assert min(lens) >= 40 and max(lens) < 80 and 55 < np.mean(lens) < 65
    assert not big.endswith(b"\n") and len(big) % 16 == 7
    assert set(M.staged(big)) == {True, False}                  # waves on both sides of SPAN


def test_span_texts():
    for span in (M.SPAN, M.SPAN + 1):
        for res in (0, 15):
            t = M.span_text(span, res)
            assert M.n_lines_of(t) == 128
            assert M.span_bytes(t)[1] == span
            assert int(M.line_starts(t)[63]) % 16 == res
            assert M.staged(t) == [True, span <= M.SPAN]
    t = M.long_previous_line_text()
    st = M.line_starts(t)
    assert M.staged(t) == [False, False] and int(st[128] - st[64]) < 2048
    assert int(st[64] - st[63]) == 5001
    t = M.long_middle_line_text()
    assert M.staged(t) == [False, True] and max(map(len, M.lines_of(t)[:30])) < 100
    for n in M.LINE_COUNTS:
        assert M.n_lines_of(M.counted_text(n)) == n and all(M.staged(M.counted_text(n)))
    t = M.counted_text(65, last_newline=False)
    assert M.n_lines_of(t) == 65 and t.count(b"\n") == 64
    assert M.wave_spans(t)[1][1] == len(t)                        # s1 = len for lane 0 of wave 1
    t = M.counted_text(200)
    assert len(M.wave_spans(t, 64)) == 1 and len(M.wave_spans(t, 65)) == 2
    assert M.wave_spans(t, 65)[1][1] == int(M.line_starts(t)[65])


def test_id_texts():
    T = M.block_first_id_texts()
    for kind, t in T.items():
        ids = O.fp_parse(t)[0]
        for l in (64, 256):
            assert (ids[l] != ids[l - 1]) == (kind == "differs")
        assert len(M.heads(ids)) == 10
    ids = O.fp_parse(M.id_pair_text())[0]
    pairs = list(zip(ids, ids[1:]))
    for n in range(1, 10):
        assert any(len(a) == len(b) == n and a[:-1] == b[:-1] and a != b for a, b in pairs)
        assert any(len(a) == len(b) == n and a == b for a, b in pairs)
    for n in range(1, 9):
        assert any(len(a) == n and len(b) == n + 1 and b.startswith(a) for a, b in pairs)
        assert any(len(b) == n and len(a) == n + 1 and a.startswith(b) for a, b in pairs)
    off = O.fp_parse_arrays(M.id_residue_text())[0].astype(np.int64)
    assert {int(a) % 4 for a in off} == {0, 1, 2, 3}
    assert len({(int(a) % 4, int(b) % 4) for a, b in zip(off, off[1:])}) >= 12


def test_grammar_texts():
    assert M.staged(M.grammar_text()) == [True]
    assert M.staged(M.grammar_text(long_line=True)) == [False]
    assert M.n_lines_of(M.grammar_text(long_line=True)) == len(M.GRAMMAR) + 1 < 64


def test_head_texts():
    for n in M.HEAD_COUNTS:
        t, hd = M.head_text(n)
        ids, vals, used = O.fp_parse(t)
        assert used == n and M.heads(ids) == hd == [h for h in M.HEAD_AT if h < n]
        assert M.head_groups(n) == (n + 1023) // 1024
    assert {h % 4 for h in M.HEAD_AT} >= {3, 0} and {1023, 1024, 1025} <= set(M.HEAD_AT)
    ids = O.fp_parse(M.all_heads_text())[0]
    assert len(ids) == 1025 and M.heads(ids) == list(range(1025))
    for n in M.ONE_REF_LINES:
        ids, vals, _u = O.fp_parse(M.one_ref_text(n))
        assert len(ids) == n and M.heads(ids) == [0]
        assert M.ref_lengths([0], [len(v) for v in vals]) == [sum(i % 5 for i in range(n))]
    for n in (1, 3, 4, 5):
        assert len(M.heads(O.fp_parse(M.n_refs_text(n))[0])) == n
    ids, vals, _u = O.fp_parse(M.doubled_first_text())
    assert M.ref_lengths(M.heads(ids), [len(v) for v in vals]) == [8, 4, 2]
    for n in M.RING_EDGE:
        t = M.alternating_text(n)
        assert len(t) == 2 * n and M.n_lines_of(t) == n and t[:4] == b"a\nb\n"
    assert M.RING_EDGE[0] * 28 <= 8 << 20 < M.RING_EDGE[1] * 28
    n = M.TWO_HEAD_SCAN_LINES
    assert n == 1_049_601 and M.scan_blocks(M.head_groups(n)) == 2
    assert M.scan_blocks(M.head_groups(n - M.HEAD_LINES - 1)) == 1 and n > M.RING_EDGE[1]
