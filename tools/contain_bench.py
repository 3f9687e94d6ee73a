#!/usr/bin/env python3
"""Contain timing at config C2's shape: the batch's sketches (10,000 x 2 kb, k = 21, s = 1000,
sketched on the device) against themselves through fpm_contain_dev, once in AUTO mode
(contain_rows_kernel) and once in forced LITERAL mode (contain_literal_kernel), and, as the
closest work the library did before contain, fpm_dist_dev16 with FPM_DIST_DENSE forced on the
same rows.  Times are the library's HIP events around the compare launches (FPM_K_COMPARE), so
the order test's read-back and dist's finalize are not in them.  The two contain grids are
fetched and compared cell for cell.  One JSON line.

    python tools/contain_bench.py [--n-seqs 10000] [--families 100] [--seq-len 2000]
                                  [--k 21] [--s 1000] [--repeat 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fp-mash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seqs", type=int, default=10000)
    ap.add_argument("--families", type=int, default=100)
    ap.add_argument("--seq-len", type=int, default=2000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()

    import fpmash
    from fpmash import datagen
    seqs = datagen.family_dna(a.families, max(1, a.n_seqs // a.families), a.seq_len,
                              sub_rate=(0.01, 0.10), seed=1000)[: a.n_seqs]
    n = len(seqs)
    P = fpmash.make_params(k=a.k, s=a.s)
    with fpmash.Context(0) as ctx:
        job = ctx.sketch_job(P, seqs)
        job.run()
        ctx.synchronize()
        d_rows, d_len, n_groups, stride = job.device_output()
        assert n_groups == n
        cells = n * n
        co = [fpmash.DeviceBuffer(ctx, cells * 4) for _ in range(2)]
        st = [fpmash.DeviceBuffer(ctx, cells * 4) for _ in range(2)]

        def contain(mode, i, rows=n):
            ctx.set_contain_mode(mode)
            ctx.contain_dev(d_rows, d_len, stride, n, d_rows, d_len, stride, rows, True,
                            co[i].ptr, st[i].ptr)
            ctx.synchronize()
            return ctx.last_contain_kernel()

        def timed(fn):
            best = None
            for _ in range(a.repeat):
                ctx.reset_timing()
                fn()
                ms = ctx.kernel_time(fpmash.K_COMPARE)[0]
                best = ms if best is None else min(best, ms)
            return best

        contain(fpmash.CONTAIN_AUTO, 0, rows=8)         # code-object load, LDS attribute
        contain(fpmash.CONTAIN_LITERAL, 1, rows=8)
        ctx.set_timing(True)
        kernels = []
        auto_ms = timed(lambda: kernels.append(contain(fpmash.CONTAIN_AUTO, 0)))
        lit_ms = timed(lambda: kernels.append(contain(fpmash.CONTAIN_LITERAL, 1)))
        ctx.set_contain_mode(fpmash.CONTAIN_AUTO)
        ctx.set_timing(False)
        same = True
        for x, y in (co, st):
            same &= bool(np.array_equal(x.to_array(np.uint32, cells), y.to_array(np.uint32, cells)))
        steps = st[0].to_array(np.uint32, cells)
        common = co[0].to_array(np.uint32, cells)
        for b in co + st:
            b.free()

        # the dense dist walk of the same rows (u16 counts, plus the finalize outputs it needs)
        lengths = fpmash.DeviceBuffer.from_array(ctx, np.full(n, a.seq_len, np.uint64))
        outs = [fpmash.DeviceBuffer(ctx, cells * b) for b in (2, 2, 8, 8, 1)]

        def dist():
            fpmash._check(fpmash.lib().fpm_dist_dev16(
                ctx.h, d_rows, d_len, lengths.ptr, stride, n, d_rows, d_len, lengths.ptr, stride,
                n, 8, a.s, a.k, 4.0 ** a.k, -1.0, -1.0, *[o.ptr for o in outs], None))
            ctx.synchronize()

        ctx.set_dist_mode(fpmash.DIST_DENSE)
        dist()
        ctx.set_timing(True)
        dist_ms = timed(dist)
        dist_kernel = ctx.last_dist_kernel()
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        for b in outs + [lengths]:
            b.free()
        job.free()
    res = {"n": n, "seq_len": a.seq_len, "k": a.k, "s": a.s, "pairs": cells,
           "contain_auto_ms": round(auto_ms, 3),
           "contain_auto_kernel": fpmash.CONTAIN_KERNELS[kernels[0]],
           "contain_literal_ms": round(lit_ms, 3),
           "dist_dense_ms": round(dist_ms, 3),
           "dist_dense_kernel": fpmash.DIST_KERNELS[dist_kernel],
           "auto_equals_literal": same,
           "mean_steps": round(float(steps.mean()), 2),
           "pairs_with_common": int((common > 0).sum()),
           "build": fpmash.lib().fpm_build_id().decode()}
    print(json.dumps(res), flush=True)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
