"""CPU tests of the bench's host-side helpers: the C++ CFL generator (C3 inputs), the -fp
line grouping of the C3 leg, and the C4 leg's query-row sharding; one GPU test of a plain
bench run's line and --dump-outputs files."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import seqio


def test_cflgen_matches_lyn2vec_fixture():
    """bin/cflgen reproduces lyn2vec's DNA1-CFL.txt from DNA1.fasta byte for byte."""
    from fpmash import datagen
    recs = seqio.read_records(os.path.join(GOLDEN, "DNA1.fasta"))
    ids = [comment.split()[0].decode()[len("G00000"):] for _name, comment, _seq in recs]
    out = datagen.cfl_text_fast([seq for _n, _c, seq in recs], ids, threads=3)
    assert out == open(os.path.join(GOLDEN, "DNA1-CFL.txt"), "rb").read()


def test_cflgen_matches_python_generator():
    """Short records (one window), lowercase, non-ACGT bytes, long records."""
    from fpmash import datagen
    seqs = datagen.random_dna(7, 350, seed=9) + [b"acgtNNacg", b"ACGTACGTAC" * 30, b"A", b"tttt" * 40]
    ids = datagen.lyn2vec_ids(len(seqs), seed=2)
    assert datagen.cfl_text_fast(seqs, ids) == datagen.cfl_text(seqs, ids)
    assert datagen.cfl_text_fast(seqs, ids, window=17) == datagen.cfl_text(seqs, ids, window=17)


def test_c4_row_shards_cover_grid():
    """The C4 leg's query-row blocks partition [0, n) for every GPU count."""
    from fpmash.shard import shard_range
    for n in (1, 7, 50_000):
        for ws in (1, 2, 3, 4, 8):
            spans = [shard_range(n, ws, r) for r in range(ws)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


def test_sub_rates_divide_by_event_timed_steps():
    """bench's sketch / dist sub-rates: kernel totals come from the event-timed steps run
    after the timed region, so per-step device time divides by their count."""
    import bench
    for steps, n in ((1, 3), (5, 5), (20, 10), (100, 10)):
        assert bench.timing_steps(steps) == n
    kt = {"a": {"total_ms": 1.8, "launches": 10, "avg_ms": 0.18},
          "b": {"total_ms": 0.2, "launches": 10, "avg_ms": 0.02}}
    ms = bench.per_step_ms(kt, ["a", "b", "missing"], bench.timing_steps(20))
    assert abs(ms - 0.2) < 1e-12          # = avg launch time summed over the kernels


def test_parity_summary():
    import bench
    p = bench.parity_summary({"ok": True}, {"parity": {"ok": True}}, None)
    assert p["all_ok"] is True and p["c4"] is None
    p = bench.parity_summary({"ok": True}, {"parity": {"ok": False}}, {"parity": None})
    assert p["all_ok"] is False


def test_c5_file_shards_balanced_by_bases():
    """bench.balanced_file_shards: contiguous file ranges covering every file once, in
    order, each rank's bases within one file of the even share."""
    import bench
    rng = np.random.default_rng(3)
    for ws in (1, 2, 3, 4, 8):
        for lengths in ([5] * 1000, list(rng.integers(1, 100, size=37)), [10, 1, 1, 1, 1, 10]):
            spans = bench.balanced_file_shards(lengths, ws)
            assert spans[0][0] == 0 and spans[-1][1] == len(lengths)
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            share = sum(lengths) / ws
            for lo, hi in spans:
                assert abs(sum(lengths[lo:hi]) - share) <= max(lengths)


def test_c5_genome_deterministic():
    import bench
    a = bench.c5_genome(7, 1001)
    assert a == bench.c5_genome(7, 1001) and a != bench.c5_genome(8, 1001)
    assert len(a) == 1001 and set(a) <= set(b"ACGT")


def test_headline_line_fits_driver_parser():
    """The printed line is built from the full result by compact_line and stays under the
    driver's parse limit (round 3's 26.8 KB line was not parsed).  Canned input: the full
    result of the round-3 bench, which carries every leg."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = json.load(open(os.path.join(root, "profiles", "r03", "bench_r03_head_final.json")))
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) < bench.MAX_LINE_BYTES
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype",
              "config", "roofline", "cpu_baseline", "parity", "higher_is_better", "scaling",
              "vs_baseline", "data"):
        assert k in line, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert line["parity"]["all_ok"] is True
    assert all(isinstance(v, (bool, type(None))) for v in line["parity"].values())
    assert line["legs"]["c4_ms_per_step"] > 0 and line["legs"]["cli_dist_wall_s"] > 0
    # a pathological detail (huge strings) still yields a parseable line
    full["cpu_baseline"]["sample"] = "x" * 20000
    assert len(json.dumps(bench.compact_line(full))) < bench.MAX_LINE_BYTES


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    """A plain run is the default: --full and --dump-outputs are options."""
    import sys
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_outputs(tmp_path, oracle):
    """A plain `bench.py --dump-outputs DIR` run (a small batch whose sketches are shorter than
    s): the line carries the headline fields and no leg, and the dumped arrays, float32 /
    float64 under 64 MB in all, equal the oracle's sketches, shared-hash counts and listed
    cells (distance and p-value within rtol 1e-12, the suite's tolerance for both)."""
    import json
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shape = dict(n_seqs=300, seq_len=600, families=3)
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--n-seqs", "300", "--seq-len", "600",
                        "--families", "3", "--dump-outputs", str(out)],
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "bases/s" and line["higher_is_better"] is True
    assert abs(line["value"] - 300 * 600 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["legs"] == {} and line["cpu_baseline"] is None
    assert line["parity"]["all_ok"] is None
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) < 64 << 20

    n, s, k = 300, 1000, 21
    seqs = bench.make_batch(bench.parse_args_for_test(**shape), 0)
    exp = oracle.sketch_batch(oracle.params(k=k, s=s), seqs)
    assert max(len(e) for e in exp) < s
    assert np.array_equal(d["sketch_counts"], [len(e) for e in exp])
    rows = d["sketch_rows"].astype(np.int64)
    assert np.array_equal(rows, np.arange(n))          # a batch this small is dumped whole
    got = (d["sketch_hash_hi"].astype(np.uint64) << np.uint64(32)) | \
        d["sketch_hash_lo"].astype(np.uint64)
    for r in rows:
        assert np.array_equal(got[r, :len(exp[r])], exp[r]) and not got[r, len(exp[r]):].any()

    lengths = [600] * n
    nu, de, di, pv = (x.reshape(n, n) for x in
                      oracle.dist_grid(exp, lengths, exp, lengths, s, k, 4.0 ** k))
    grid = d["grid_rows"].astype(np.int64)
    assert len(grid) == 200 and len(set(grid)) == 200
    assert np.array_equal(d["numer"], nu[grid]) and np.array_equal(d["denom"], de[grid])
    assert np.array_equal(d["listed_rows"], np.arange(n))
    q, r = np.nonzero(nu)                              # row-major: sorted by (query, reference)
    assert d["listed_count"][0] == len(q) > n
    assert np.array_equal(d["listed_qry"], q) and np.array_equal(d["listed_ref"], r)
    assert np.allclose(d["listed_distance"], di[q, r], rtol=1e-12, atol=0)
    assert np.allclose(d["listed_pvalue"], pv[q, r], rtol=1e-12, atol=0)
    assert np.array_equal(d["listed_pass"], np.ones(len(q)))
