"""Model of the device FASTA / FASTQ parser (csrc/seqparse.hip) and the inputs its tests share.

Three parts restate the parser in plain Python:
  * records(): the serial four-state machine (S0 before any header, S1 sequence, S2 header line,
    S3 stream ended) over one file, one byte at a time;
  * summary() / compose(): the effect of a byte range as a map over the four input states with,
    per input state, the records started, the sequence bytes kept and whether a '+' was met in
    sequence text; the kernels fold such summaries over 16-byte threads, 4096-byte chunks and the
    chunk-level scan, which is sound only if the fold is associative;
  * fastq_four_line(): the acceptance rules of the 4-line FASTQ path, record by record.
The generators below build the inputs of tests/test_gpu_seqparse_edges.py; tests/
test_seqparse_model.py pins the model, on those inputs too, to tests/seqio.py (and through it
to the reference's kseq.h)."""
import numpy as np

CHUNK = 4096            # kSpChunk: bytes per workgroup; every file starts on a chunk boundary
THREAD_BYTES = 16       # kSpBytes: bytes per thread
SCAN_THREADS = 1024     # kSpScanThreads: threads of the one-workgroup chunk scan
SCAN_BLOCK = 1024       # records per workgroup of scan64_local_kernel
SUMS_ROUND = 256        # block totals per round of scan64_sums_kernel's carry loop
S0, S1, S2, S3 = 0, 1, 2, 3
MARKERS = (62, 64)      # '>' '@'
SPACE = b" \t\n\v\f\r"


def is_seq(c):
    """a byte kept as sequence in S1: isgraph minus the bytes that end a sequence"""
    return 0x21 <= c <= 0x7E and c not in (62, 64, 43)


def step_byte(x, c):
    """state x, byte c -> (next state, a record starts at this byte)"""
    mk, eof = c in MARKERS, c == 0xFF
    start = (mk and x in (S0, S1)) or (eof and x == S1)
    if x == S3 or (eof and x == S0):
        return S3, start
    if mk or (eof and x == S1):
        return S2, start
    return (S1 if (c == 10 and x == S2) else x), start


def run(data, state=S0):
    """the machine over `data` from `state` -> (out state, records started, sequence bytes kept,
    a '+' met in sequence text)"""
    starts = kept = 0
    plus = False
    for c in data:
        if state == S1:
            kept += is_seq(c)
            plus = plus or c == 43
        state, st = step_byte(state, c)
        starts += st
    return state, starts, kept, plus


def records(data):
    """[(header position, header end or None, sequence bytes)] of one file: the header position is
    the '>' / '@' (or the 0xff that ended the record before it), the header end its '\\n' (None
    where the file ends inside the header line)"""
    out = []
    state = S0
    for i, c in enumerate(data):
        if state == S1 and is_seq(c):
            out[-1][2].append(c)
        if state == S2 and c == 10:
            out[-1][1] = i
        state, st = step_byte(state, c)
        if st:
            out.append([i, None, bytearray()])
    return [(p, e, bytes(s)) for p, e, s in out]


def split_header(line):
    """(name, comment) of a header line without its marker and its '\\n': the name ends at the
    first isspace byte, the comment is the rest behind that byte"""
    i = 0
    while i < len(line) and line[i] not in SPACE:
        i += 1
    return line[:i], (line[i + 1:] if i < len(line) else b"")


def named(data, recs):
    """[(name, comment, sequence)] as kseq_read returns the records of records(data): a marker
    that is the file's last byte starts none (the name read meets the end of the stream)"""
    out = []
    for p, e, s in recs:
        if p + 1 >= len(data):
            continue
        out.append(split_header(data[p + 1:len(data) if e is None else e]) + (s,))
    return out


# ---- summaries ------------------------------------------------------------------------

def identity():
    return tuple((s, 0, 0, False) for s in range(4))


def summary(chunk):
    """per input state: run(chunk, state)"""
    return tuple(run(chunk, s) for s in range(4))


def compose(f, g):
    """f then g"""
    out = []
    for s in range(4):
        m, ns, nk, pl = f[s]
        gm = g[m]
        out.append((gm[0], ns + gm[1], nk + gm[2], pl or gm[3]))
    return tuple(out)


def reset(f):
    """the summary of a file's first chunk: every input state behaves as S0"""
    return (f[0],) * 4


def fold(pieces):
    """the summaries of the pieces composed left to right"""
    x = identity()
    for p in pieces:
        x = compose(x, summary(p))
    return x


def n_chunks(files):
    """chunks of one parse: each file from a chunk boundary with at least one '\\n' behind it"""
    return sum((len(f) + 1 + CHUNK - 1) // CHUNK for f in files)


# ---- 4-line FASTQ ---------------------------------------------------------------------

def fastq_four_line(data):
    """The records [(name, comment, sequence)] of one file where every record passes the rules
    of the device's 4-line FASTQ path, else None (the device hands the parse to the host).
    The rules, per record of four lines (header, sequence, '+', quality):
      * the header line starts with a marker (the file's first record: at the file's first
        byte) and its '\\n' is inside the file;
      * the sequence line holds no marker, '+' or 0xff; its isgraph bytes are the bases;
      * the third line starts with '+', holds no 0xff and its '\\n' is inside the file;
      * the quality line holds the base count of bytes in 33..127 with no 0xff up to the last
        of them; the byte behind that one is consumed; no marker or 0xff follows on the line;
      * the lines after the last record hold no marker."""
    n = len(data)
    text = data + b"\n"                         # the '\n' padding behind every file
    starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10]
    n_lines = sum(1 for s in starts if s < n)
    out = []
    for r in range(n_lines // 4):
        L = 4 * r
        h0, h1 = starts[L], starts[L + 1] - 1
        s0, s1 = h1 + 1, starts[L + 2] - 1
        p0, p1 = s1 + 1, starts[L + 3] - 1
        q0, q1 = p1 + 1, starts[L + 4] - 1
        if not (text[h0] in MARKERS and h1 < n and text[p0] == 43 and p1 < n):
            return None
        line = text[s0:s1]
        if any(c in MARKERS or c in (43, 0xFF) for c in line):
            return None
        seq = bytes(c for c in line if 0x21 <= c <= 0x7E)
        if 0xFF in text[p0 + 1:p1]:
            return None
        i = q0
        if seq:
            v = 0
            while i < q1:
                c = text[i]
                if c == 0xFF:
                    return None
                if 33 <= c <= 127:
                    v += 1
                    if v == len(seq):
                        break
                i += 1
            if v != len(seq):
                return None
            i += 1
        if any(c in MARKERS or c == 0xFF for c in text[i + 1:q1]):
            return None
        out.append(split_header(text[h0 + 1:h1]) + (seq,))
    if any(c in MARKERS for c in data[starts[n_lines // 4 * 4]:]):
        return None
    return out


def device_parse(data):
    """What one parse of the single file `data` must report -> (records, quality flag): the
    machine's records where no '+' is met in sequence text, else the 4-line records, else
    (None, True): the caller walks the file on the host."""
    if not run(data)[3]:
        return named(data, records(data)), False
    recs = fastq_four_line(data)
    return (recs, False) if recs is not None else (None, True)


# ---- generators -----------------------------------------------------------------------

ALPHABET = b">>@@\n\n\n\r \t\x00\xff\xff\x7fACGTNacgt"   # weighted to the bytes that change state


def random_strings(seed, count, max_len=40):
    """`count` strings of 0..max_len bytes over ALPHABET (no '+': the four-state machine)"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(ALPHABET, np.uint8)
    lens = rng.integers(0, max_len + 1, count)
    flat = alpha[rng.integers(0, len(alpha), int(lens.sum()))].tobytes()
    at = 0
    for n in lens:
        yield flat[at:at + n]
        at += n


def bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def seq_lines(rng, n, width=61):
    """n bytes of sequence text: bases in lines of `width` (the '\\n' bytes count)"""
    s = bytearray(bases(rng, n))
    s[width - 1::width] = b"\n" * len(s[width - 1::width])
    return bytes(s)


def header_fill(rng, n):
    """n header bytes: words with spaces, tabs, '>' and '@' (ordinary inside a header), no '\\n'"""
    return np.frombuffer(b"abcdefgh01234 \t>@_.", np.uint8)[rng.integers(0, 19, n)].tobytes()


def preamble_fill(rng, n):
    """n marker-free bytes before any header: text lines"""
    return np.frombuffer(b"acgtACGT xyz\n\r\t\x00", np.uint8)[rng.integers(0, 16, n)].tobytes()


def fasta_records(rng, n_rec, lo, hi, width=61, tag=b"r"):
    out = bytearray()
    for i in range(n_rec):
        out += b">%s%d c %d\n" % (tag, i, i) + seq_lines(rng, int(rng.integers(lo, hi + 1)), width)
        out += b"\n"
    return bytes(out)


PRIORS = ("S0", "S1", "S2", "S2ff")
# the byte(s) placed on the boundary; what they do depends on the prior state: '>' / '@' start a
# record from S0 / S1 and are header text in S2; '\n' / "\r\n" end the header line in S2; 0xff
# ends the stream from S0, starts a record from S1, is header text in S2; a space is dropped
# from sequence text in S1
EVENTS = (b">", b"@", b"\n", b"\r\n", b"\xff", b" ")
EVENT_OFFSETS = (15, 16, 17, 1023, 1024, 4095, 4096, 4097, 8191, 8192)
EVENT_TAIL = b"GATTACA\nTTG CA\n>t1 tail rec\nACGTTGCA\nAC\n>t2\nGG\n"


def prior_text(rng, prior, n):
    """n bytes that leave the machine in the prior state (n >= 15)"""
    if prior == "S0":
        return preamble_fill(rng, n)
    if prior == "S1":
        head = b">p1 c\n"
        return head + seq_lines(rng, n - len(head))
    if prior == "S2":
        return b">" + header_fill(rng, n - 1)
    head = b">a\nACGT\xff"
    return head + header_fill(rng, n - len(head))


def event_files():
    """[(prior, event, offset, file)]: the event's first byte at in-file offset `offset`, the
    part before it padded to that length, EVENT_TAIL behind it"""
    rng = np.random.default_rng(21)
    out = []
    for prior in PRIORS:
        for ev in EVENTS:
            for off in EVENT_OFFSETS:
                out.append((prior, ev, off, prior_text(rng, prior, off) + ev + EVENT_TAIL))
    return out


def long_run_files():
    """{name: file} in parse order, the runs longer than a chunk and the file-end cases"""
    rng = np.random.default_rng(22)
    well_formed = fasta_records(rng, 12, 1000, 2400)            # about 5 chunks
    assert 4.5 * CHUNK < len(well_formed) < 6 * CHUNK
    files = {
        "long header": b">" + header_fill(rng, int(3.2 * CHUNK)) + b"\nACGTTGCAAC\n>n x\nAC\n",
        "long preamble": preamble_fill(rng, int(2.5 * CHUNK)) + fasta_records(rng, 3, 0, 90),
        "long record": b">long one\n" + bases(rng, 5 * CHUNK + 7) + b"\n",
        "stream ended": b"\xff" + well_formed,
        "after stream ended": fasta_records(rng, 4, 0, 200, tag=b"n"),
        "ends in header": b">a\nAC\n>tail no newline",
        "after ends in header": b">b\nGGT\n",
    }
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        head = b">e%d\n" % n
        files["ends in sequence %d" % n] = head + bases(rng, n - len(head))
        files["after ends in sequence %d" % n] = b"ACGT\n>f%d z\nTTGCA" % n   # preamble, record
    files["before empty"] = b">x\nAC"
    files["empty"] = b""
    files["after empty"] = b">y\nGT\n"
    return files


def tiny_pool():
    """about 20 file contents of a few dozen bytes, one or two records each, with a file whose
    stream ends at once (S3), a header-only file and an empty file"""
    rng = np.random.default_rng(23)
    pool = [b"", b"\xff>dead\nACGT\n", b">only header", b"x\xff\n>dead2\nAC\n", b">"]
    for i in range(16):
        f = b">p%d c\n" % i + bases(rng, int(rng.integers(0, 30))) + b"\n"
        if i % 2:
            f += b"@q%d\n" % i + bases(rng, int(rng.integers(1, 20)))
        if i % 5 == 0:
            f = b"pre\n" + f
        pool.append(f)
    return pool


def partition_files(n):
    """The files of one chunk-scan case of exactly n chunks -> (files, [(first chunk, chunks)] of
    the three multi-chunk files).  The scan gives thread t the chunks [t * per, (t + 1) * per),
    per = ceil(n / 1024); the multi-chunk files (5, 6 and 7 chunks: sequence, a header line and
    an ended stream carried across chunks) start at chunk indices that are per - 1, 1 and
    per - 1 modulo per, so each crosses at least one range edge away from its own first chunk.
    Every other file is one chunk from tiny_pool(); the last file holds records."""
    rng = np.random.default_rng(24)
    per = (n + SCAN_THREADS - 1) // SCAN_THREADS
    big = [
        b">s1 carried\n" + bases(rng, 4 * CHUNK + 100) + b"\n>s1b\nACG\n",             # 5 chunks
        b">" + header_fill(rng, 5 * CHUNK + 33) + b"\nACGTAC\n>s2b\nTT\n",              # 6 chunks
        b"junk\n\xff" + fasta_records(rng, 26, 1000, 2400)[:6 * CHUNK + 500],          # 7 chunks
    ]
    assert [n_chunks([b]) for b in big] == [5, 6, 7]

    def at_least(lo, rem):
        return lo + (rem - lo) % per

    where = [at_least(100, per - 1), at_least(n // 2, 1 % per), at_least(n - 40, per - 1)]
    pool = tiny_pool()
    files, spans, c = [], [], 0
    while c < n - 1:
        if where and c == where[0]:
            where.pop(0)
            files.append(big[len(spans)])
            spans.append((c, n_chunks(files[-1:])))
            c += spans[-1][1]
        else:
            files.append(pool[int(rng.integers(0, len(pool)))])
            c += 1
    files.append(b">last rec\nACGTTGCA\nGG\n>very last\nT\n")
    return files, spans


# ---- FASTQ generators -----------------------------------------------------------------

WINDOW_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


def quality_for(rng, n):
    """n counted quality bytes (33..127) with '@', '>' and 0x7f among them"""
    q = rng.integers(33, 128, n).astype(np.uint8)
    q[q == 43] = 44                              # no '+' needed; keep the line unambiguous
    if n > 2:
        q[1::7] = 64
        q[2::11] = 62
        q[n // 2] = 0x7F
    return q.tobytes()


def fastq_record(name, line, rng, nl=b"\n"):
    """one 4-line record whose sequence line is `line` (spaces, tabs, '\\r', 0x7f allowed: not
    bases); the quality line holds one counted byte per base"""
    n = sum(1 for c in line if 0x21 <= c <= 0x7E)
    return b"@" + name + nl + line + nl + b"+" + nl + quality_for(rng, n) + nl


def window_lines(rng):
    """[(tag, sequence line)]: the shapes of test_fastq_emit_windows"""
    out = []
    for n in WINDOW_LENGTHS:
        out.append((b"b%d" % n, bases(rng, n, b"ACGTN")))
        out.append((b"cr%d" % n, bases(rng, n, b"ACGTN") + b"\r"))
        line = bytearray(bases(rng, n, b"ACGTN"))
        for k, p in enumerate((0, 31, 32, 63)):
            if p < n:
                line[p] = b" \t"[k & 1]
        out.append((b"sp%d" % n, bytes(line)))
    line = bytearray(bases(rng, 200, b"ACGTN"))
    line[2::3] = bytes(b" \t\x00\x7f"[i & 3] for i in range(len(line[2::3])))
    out.append((b"third", bytes(line)))
    line = bytearray(bases(rng, 150, b"ACGTN"))
    line[0] = line[63] = line[64] = line[65] = line[127] = line[149] = 0x7F
    out.append((b"del", bytes(line)))
    return out


def window_files():
    """two FASTQ files of the window_lines() shapes: '\\n' lines, and CRLF throughout"""
    rng = np.random.default_rng(25)
    lines = window_lines(rng)
    return [b"".join(fastq_record(t + b" lf", ln, rng) for t, ln in lines),
            b"".join(fastq_record(t + b" crlf", ln, rng, b"\r\n") for t, ln in lines)]


SCAN_FILE_RECORDS = (1023, 1, 0, 1025, 2048, 0)


def fastq_reads(rng, n_rec, lo, hi, tag):
    """-> (file, [(name, comment, sequence)]): n_rec 4-line records of lo..hi bases"""
    out, recs = [], []
    for i in range(n_rec):
        s = bases(rng, int(rng.integers(lo, hi + 1)), b"ACGTN")
        name = b"%s%d" % (tag, i)
        out.append(b"@%s len=%d\n%s\n+\n%s\n" % (name, len(s), s, quality_for(rng, len(s))))
        recs.append((name, b"len=%d" % len(s), s))
    return b"".join(out), recs


def scan_files():
    """-> (files, per file [(name, comment, sequence)]): FASTQ files of SCAN_FILE_RECORDS
    records with irregular read lengths, an empty file in the middle and at the end"""
    rng = np.random.default_rng(26)
    made = [fastq_reads(rng, n, 0, 40, b"f%d_" % i) for i, n in enumerate(SCAN_FILE_RECORDS)]
    return [m[0] for m in made], [m[1] for m in made]


BIG_FASTQ_RECORDS = SCAN_BLOCK * SUMS_ROUND + 1 + 1000      # a 257th block total: two rounds


def big_fastq():
    """-> (file, names, sequences): BIG_FASTQ_RECORDS minimal 4-line records, 0..3 bases each,
    the name one letter; the records are the generator's own"""
    rng = np.random.default_rng(27)
    n = BIG_FASTQ_RECORDS
    lens = rng.integers(0, 4, n)
    letters = rng.integers(0, 26, n)
    flat = bases(rng, int(lens.sum()))
    out, names, seqs, at = [], [], [], 0
    for i in range(n):
        s = flat[at:at + lens[i]]
        at += lens[i]
        nm = b"abcdefghijklmnopqrstuvwxyz"[letters[i]:letters[i] + 1]
        out.append(b"@%s\n%s\n+\n%s\n" % (nm, s, b"@~>"[:len(s)]))
        names.append(nm)
        seqs.append(s)
    return b"".join(out), names, seqs
