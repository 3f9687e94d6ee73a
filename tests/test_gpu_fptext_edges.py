"""The -fp text path on the device (csrc/fingerprint.hip, the -fp half of csrc/fpm_text_api.cpp)
at its chunk, span and head-scan edges.  Every comparison is exact and on every field:
Context.fp_text's ID bytes, value count, hash and new-ID flag per line, and Context.fp_refs'
first lines, ID bytes, lengths, hashes and line count, for 32- and 64-bit hashes, against
oracle.fp_parse (held to libstdc++'s istream by tests/test_fptext_model.py) and the grouping
restated in tests/fptext_model.py.  The inputs come from that model, whose CPU tests show that
each sits on the edge it is named for; the counts that put it there are asserted again here."""
import numpy as np
import pytest

import fptext_model as M

pytestmark = pytest.mark.gpu

WIDTHS = pytest.mark.parametrize("use64", [False, True], ids=["u32", "u64"])
_hashes = {}


def line_hash(oracle, v, use64):
    key = (v.tobytes(), use64)
    if key not in _hashes:
        _hashes[key] = oracle.get_hash_fp(v, 42, use64)
    return _hashes[key]


def check_text(ctx, oracle, text, use64, cap=1_000_000, c=None):
    """fp_text and fp_refs of one text against the oracle's parse, on every field; c: the
    context (default: the session's).  -> (ids, values) of the parse"""
    c = ctx if c is None else c
    ids, vals, used = oracle.fp_parse(text, limit=cap)
    assert used == M.n_lines_of(text, cap)
    want_h = np.array([line_hash(oracle, v, use64) for v in vals], np.uint64)
    want_nv = np.array([len(v) for v in vals], np.int64)
    got = c.fp_text(text, max_lines=cap, seed=42, use64=use64)
    assert len(got["id_off"]) == len(got["hash"]) == len(got["new_id"]) == used
    assert got["hash"].dtype == (np.uint64 if use64 else np.uint32)
    got_ids = [text[int(o):int(o) + int(n)] for o, n in zip(got["id_off"], got["id_len"])]
    assert got_ids == ids
    # an empty ID has no bytes to compare: its offset is where the oracle puts it too
    assert np.array_equal(got["id_off"], oracle.fp_parse_arrays(text, limit=cap)[0])
    assert np.array_equal(got["n_vals"], want_nv)
    assert np.array_equal(got["hash"].astype(np.uint64), want_h)
    hd = M.heads(ids)
    want_new = np.zeros(used, np.uint8)
    if used:
        want_new[hd] = 1
        want_new[0] = 2
    assert np.array_equal(got["new_id"], want_new)
    refs = c.fp_refs(text, max_lines=cap, seed=42, use64=use64)
    assert refs["n_lines"] == used
    assert list(refs["first"]) == hd
    assert [text[int(o):int(o) + int(n)] for o, n in zip(refs["id_off"], refs["id_len"])] == \
        [ids[a] for a in hd]
    assert [int(x) for x in refs["length"]] == M.ref_lengths(hd, want_nv)
    assert np.array_equal(refs["hash"].astype(np.uint64), want_h)
    return ids, vals


def test_limits():
    """the constants the inputs are built for: a moved one fails here, not by moving coverage"""
    import fpmash
    assert fpmash.fp_text_limits() == (4096, 4096, 1024) == (M.TEXT_CHUNK, M.SPAN, M.HEAD_LINES)


# ---- newline index --------------------------------------------------------------------

@WIDTHS
def test_newline_text_lengths(ctx, oracle, use64):
    """texts of 1..80 bytes and either side of one and two chunks, ending 0..15 bytes into the
    last 16-byte load: all '\\n', filler with '\\n' last, filler without"""
    for (n, kind), text in M.nl_length_texts().items():
        ids, _vals = check_text(ctx, oracle, text, use64)
        assert len(ids) == (n if kind == "all" else 1), (n, kind)


@WIDTHS
def test_newline_positions(ctx, oracle, use64):
    """the one '\\n' of a 4,200-byte text at every byte of the first four threads' loads and
    either side of the chunk edge"""
    for p, text in M.nl_position_texts().items():
        ids, _vals = check_text(ctx, oracle, text, use64)
        assert [len(i) for i in ids] == [p, 4200 - p - 1], p


@WIDTHS
def test_newline_full_chunk(ctx, oracle, use64):
    """4,096 '\\n' in a chunk: every thread counts 16, the wave and block prefixes at their
    largest"""
    ids, _vals = check_text(ctx, oracle, M.nl_full_chunk(), use64)
    assert len(ids) == 8197


@pytest.mark.parametrize("n", M.STALE_LENGTHS)
def test_newline_stale_padding(oracle, n):
    """The text buffer is text_len + 16 bytes from the context's pool and only text_len bytes
    are copied, so the bytes nl_flags16 masks are whatever the block held before.  A best-effort
    provocation (which block the pool hands back cannot be observed; the assertions hold either
    way): on a fresh context, parse and free an all-'\\n' text of n + 15 bytes, whose buffer is
    the smallest block the next text's fits, then parse n filler bytes: exactly one line.  For
    the shortest texts the smallest fitting block is the first job's 24-byte chunk-count block
    instead, so a second fresh context first parses ten '\\n': that block then holds the counts
    10, 0, 10, a 0x0A at byte 8."""
    import fpmash
    first = [b"\n" * (n + 15)] + ([b"\n" * 10] if n + 16 <= 24 else [])
    for use64 in (False, True):
        for text in first:
            with fpmash.Context(0) as c:
                assert len(c.fp_text(text, use64=use64)["hash"]) == len(text)
                ids, _vals = check_text(None, oracle, b"x" * n, use64, c=c)
                assert ids == [b"x" * n]


@WIDTHS
def test_newline_two_scan_blocks(ctx, oracle, use64):
    """1,025 full chunks and 7 bytes: 1,026 chunk counts, so the scan of the counts folds two
    scan blocks; ~60-byte lines, the last one without '\\n'"""
    text = M.two_scan_blocks_text()
    assert M.scan_blocks(M.chunks(text)) == 2
    ids, _vals = check_text(ctx, oracle, text, use64)
    assert len(ids) > 65_000 and ids[-1] == b"tail"


# ---- line kernel spans ----------------------------------------------------------------

@WIDTHS
@pytest.mark.parametrize("residue", [0, 15])
@pytest.mark.parametrize("span", [M.SPAN, M.SPAN + 1])
def test_span_edge(ctx, oracle, use64, span, residue):
    """wave 1's span exactly 4,096 bytes (the last staged size: the copy loop's last 16-byte
    step fills the span array's last bytes) and 4,097 (the first global one), with the line
    before the wave starting on and 15 bytes into a 16-byte block"""
    text = M.span_text(span, residue)
    assert M.span_bytes(text)[1] == span and M.staged(text)[1] == (span == M.SPAN)
    check_text(ctx, oracle, text, use64)


@WIDTHS
def test_span_long_lines(ctx, oracle, use64):
    """a wave of short lines that reads global memory only because the line before it is over
    4,096 bytes; a 5,000-byte line among short ones"""
    text = M.long_previous_line_text()
    assert M.staged(text) == [False, False]
    check_text(ctx, oracle, text, use64)
    text = M.long_middle_line_text()
    assert M.staged(text) == [False, True]
    _ids, vals = check_text(ctx, oracle, text, use64)
    assert len(vals[30]) == 238


@WIDTHS
def test_line_counts(ctx, oracle, use64):
    """1 line to 257: a wave and a block short of, at and over full; 65 lines where the last
    has no '\\n' (lane 0 of a second wave, its span ending at the text's end); a line cap that
    ends on a wave's last lane and on the next wave's first"""
    for n in M.LINE_COUNTS:
        assert len(check_text(ctx, oracle, M.counted_text(n), use64)[0]) == n
    assert len(check_text(ctx, oracle, M.counted_text(65, last_newline=False), use64)[0]) == 65
    for cap in (64, 65):
        assert len(check_text(ctx, oracle, M.counted_text(200), use64, cap=cap)[0]) == cap


@WIDTHS
def test_ids(ctx, oracle, use64):
    """the ID of a wave's and a block's first line (64, 256) equal to and different from the line
    before; IDs of equal length differing in the last byte; IDs that are a prefix of their
    neighbour; IDs starting at every byte of a 4-byte word behind blanks and tabs"""
    for kind, text in M.block_first_id_texts().items():
        ids, _vals = check_text(ctx, oracle, text, use64)
        assert (ids[64] != ids[63]) == (ids[256] != ids[255]) == (kind == "differs")
    check_text(ctx, oracle, M.id_pair_text(), use64)
    check_text(ctx, oracle, M.id_residue_text(), use64)


# ---- value grammar --------------------------------------------------------------------

@WIDTHS
@pytest.mark.parametrize("long_line", [False, True], ids=["staged", "global"])
def test_value_grammar(ctx, oracle, use64, long_line):
    """u64 overflow to the digit, signs, tokens that end a line's values, NUL, every space byte,
    0..17 values, blank lines: from LDS, and in the same wave as a 5,000-byte line from
    global memory"""
    text = M.grammar_text(long_line)
    assert M.staged(text) == [not long_line]
    _ids, vals = check_text(ctx, oracle, text, use64)
    by_name = dict(zip([n for n, _l in M.GRAMMAR], vals[:20] + vals[20 + long_line:]))
    assert list(by_name["u64 max - 5 + 5"]) == [1, 2 ** 64 - 1, 2]
    assert list(by_name["u64 max - 5 + 6"]) == [1]
    assert len(by_name["17 values"]) == 17


# ---- heads and References -------------------------------------------------------------

@WIDTHS
def test_heads(ctx, oracle, use64):
    """line counts around one and two head-count workgroups, heads on the workgroup edge and on
    a thread's last and first line; every line a head; one Reference of 64..1,025 lines (one
    wave sums it in 1..17 steps); 1..5 References (the length kernel takes 4 to a workgroup);
    a first line of 3 values, counted twice"""
    for n in M.HEAD_COUNTS:
        text, hd = M.head_text(n)
        ids, _vals = check_text(ctx, oracle, text, use64)
        assert M.heads(ids) == hd
    check_text(ctx, oracle, M.all_heads_text(), use64)
    for n in M.ONE_REF_LINES:
        check_text(ctx, oracle, M.one_ref_text(n), use64)
    for n in (1, 3, 4, 5):
        check_text(ctx, oracle, M.n_refs_text(n), use64)
    check_text(ctx, oracle, M.doubled_first_text(), use64)


def check_alternating(ctx, oracle, n, use64, cap):
    """fp_text and fp_refs of n lines 'a' / 'b' in turn: every field, by numpy (a line
    without values hashes to one constant)"""
    text = M.alternating_text(n)
    h0 = oracle.get_hash_fp(np.zeros(0, np.uint64), 42, use64)
    buf = np.frombuffer(text, np.uint8)
    got = ctx.fp_text(text, max_lines=cap, seed=42, use64=use64)
    assert len(got["hash"]) == n
    assert np.array_equal(got["id_off"], 2 * np.arange(n, dtype=np.uint64))
    assert (got["id_len"] == 1).all() and not got["n_vals"].any()
    assert np.array_equal(buf[got["id_off"].astype(np.int64)], np.tile([97, 98], n // 2 + 1)[:n])
    assert (got["hash"] == h0).all()
    assert got["new_id"][0] == 2 and (got["new_id"][1:] == 1).all()
    refs = ctx.fp_refs(text, max_lines=cap, seed=42, use64=use64)
    assert refs["n_lines"] == n and len(refs["first"]) == n
    assert np.array_equal(refs["first"], np.arange(n, dtype=np.uint64))
    assert np.array_equal(refs["id_off"], 2 * np.arange(n, dtype=np.uint64))
    assert (refs["id_len"] == 1).all() and not refs["length"].any()
    assert (refs["hash"] == h0).all()


@WIDTHS
@pytest.mark.parametrize("n", M.RING_EDGE)
def test_refs_ring_edge(ctx, oracle, use64, n):
    """299,593 References: the last count whose four arrays fit the pinned ring in one copy;
    299,594: the first fetched array by array"""
    assert (n * 28 <= 8 << 20) == (n == M.RING_REFS)
    check_alternating(ctx, oracle, n, use64, 1_000_000)


@WIDTHS
def test_refs_two_head_scan_blocks(ctx, oracle, use64):
    """1,049,601 lines: 1,026 head counts, so their scan folds two scan blocks; every line a
    Reference (fetched array by array), and max_lines above the default million"""
    n = M.TWO_HEAD_SCAN_LINES
    assert M.scan_blocks(M.head_groups(n)) == 2
    check_alternating(ctx, oracle, n, use64, 2_000_000)


# ---- fp_hash_lines --------------------------------------------------------------------

@WIDTHS
@pytest.mark.parametrize("n", [255, 256, 257])
def test_fp_hash_lines_block_edge(ctx, oracle, use64, n):
    rng = np.random.default_rng(n)
    lines = [rng.integers(0, 2 ** 64, int(k), dtype=np.uint64) for k in rng.integers(0, 18, n)]
    got = ctx.fp_hash_lines(lines, seed=42, use64=use64)
    assert got.dtype == (np.uint64 if use64 else np.uint32)
    assert [int(x) for x in got] == [oracle.get_hash_fp(v, 42, use64) for v in lines]
