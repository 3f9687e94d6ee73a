"""The u32 exclusive scan every table build, index build and text pass goes through
(csrc/dist_index.hip: launch_exscan, reached by itself through fpm_exscan_dev) against
numpy.cumsum in uint64, exact.

B is the scan's block (elements per workgroup) and F the most blocks its two-launch form takes,
both from fpm_scan_limits: up to F * B elements scan_add_fold_kernel folds the block totals
itself (a block folds up to F - 1 of them), past that scan_sums_kernel, one workgroup walking the
totals in chunks of 256, runs between scan_local_kernel and scan_add_kernel.  The sizes sit on the
block edge, on the 256-total chunk edge (in both forms: the fold form only sums them), on either
side of F * B, and on the chunk edge of scan_sums_kernel, which only sees sizes past F * B.
"""
import numpy as np
import pytest

import fpmash

pytestmark = pytest.mark.gpu

B, F = fpmash.scan_limits()
CHUNK = 256                     # block totals scan_sums_kernel takes per step (its workgroup)
SIZES = [0, 1, B - 1, B, B + 1, (CHUNK - 1) * B + 1, CHUNK * B, CHUNK * B + 1,
         F * B - 1, F * B, F * B + 1,
         F * B + CHUNK * B - 1, F * B + CHUNK * B, F * B + CHUNK * B + 1,
         F * B + (CHUNK + 1) * B + 3]
PAD = B + 7                     # cells allocated past n: a whole block and a ragged bit
POISON_BYTE = 0xA5
POISON = np.uint32(0xA5A5A5A5)


def inputs(n):
    """(name, u32 array of n counts) of the three families"""
    rng = np.random.default_rng(n + 1)
    out = [("random", rng.integers(0, 8, size=n, dtype=np.uint32))]
    ones = {"one at 0": 0, "one at the end": n - 1}
    if n > F * B:
        ones["one at block F"] = F * B
    for name, at in ones.items():
        if n:
            x = np.zeros(n, np.uint32)
            x[at] = 1
            out.append((name, x))
    if n:
        # a few large values over many blocks, zeros elsewhere, 2^32 - 1 in all: every carry at
        # full width and none wraps
        at = np.unique(np.linspace(0, n - 1, min(n, 13)).astype(np.int64))
        part = (2 ** 32 - 1) // len(at)
        x = np.zeros(n, np.uint32)
        x[at] = part
        x[at[-1]] += (2 ** 32 - 1) - part * len(at)
        assert int(x.sum(dtype=np.uint64)) == 2 ** 32 - 1
        out.append(("total 2^32 - 1", x))
    return out


def reference(x):
    """-> (the exclusive scan, the total), through uint64 and shown to fit u32"""
    cs = np.cumsum(x, dtype=np.uint64)
    total = int(cs[-1]) if len(x) else 0
    assert total < 2 ** 32
    ex = np.zeros(len(x), np.uint64)
    ex[1:] = cs[:-1]
    return ex.astype(np.uint32), total


@pytest.fixture(scope="module")
def bufs(ctx):
    """device buffers for the largest size: in, out, out2 (n + PAD cells each) and the total's
    four cells"""
    cells = max(SIZES) + PAD
    b = {k: fpmash.DeviceBuffer(ctx, cells * 4) for k in ("in", "out", "out2")}
    b["total"] = fpmash.DeviceBuffer(ctx, 16)
    yield b
    for v in b.values():
        v.free()


def test_limits_without_a_device_argument():
    assert B >= 4 and F >= 1
    fpmash.lib().fpm_scan_limits(None, None)
    # the sizes named for the three-launch form take it
    assert [n > F * B for n in SIZES] == [False] * 10 + [True] * 5


def test_refusals(ctx, bufs):
    L = fpmash.lib()
    p = bufs["in"].ptr
    assert L.fpm_exscan_dev(ctx.h, None, 5, p, None, None) == fpmash.FPM_EINVAL
    assert L.fpm_exscan_dev(ctx.h, p, 5, None, None, None) == fpmash.FPM_EINVAL
    assert L.fpm_exscan_dev(None, p, 5, p, None, None) == fpmash.FPM_EINVAL
    assert L.fpm_exscan_dev(ctx.h, p, 2 ** 31 + 1, p, None, None) == fpmash.FPM_EINVAL
    assert L.fpm_exscan_dev(ctx.h, None, 0, None, None, None) == fpmash.FPM_OK


@pytest.mark.parametrize("n", SIZES)
def test_exscan(ctx, bufs, n):
    L = fpmash.lib()
    cells = n + PAD
    for name, x in inputs(n):
        want, want_total = reference(x)
        fpmash._check(L.fpm_memset(ctx.h, bufs["in"].ptr, POISON_BYTE, cells * 4))
        if n:
            fpmash._check(L.fpm_memcpy_h2d(ctx.h, bufs["in"].ptr, x.ctypes.data, x.nbytes))
        for with_out2 in (False, True):
            for with_total in (False, True):
                for k in ("out", "out2"):
                    fpmash._check(L.fpm_memset(ctx.h, bufs[k].ptr, POISON_BYTE, cells * 4))
                fpmash._check(L.fpm_memset(ctx.h, bufs["total"].ptr, POISON_BYTE, 16))
                ctx.exscan_dev(bufs["in"].ptr, n, bufs["out"].ptr,
                               bufs["out2"].ptr if with_out2 else None,
                               bufs["total"].ptr if with_total else None)
                what = f"n={n} {name} out2={with_out2} total={with_total}"
                out = bufs["out"].to_array(np.uint32, cells)
                out2 = bufs["out2"].to_array(np.uint32, cells)
                tot = bufs["total"].to_array(np.uint32, 4)
                assert np.array_equal(out[:n], want), what
                assert (out[n:] == POISON).all(), what
                if with_out2:
                    assert np.array_equal(out2[:n], want), what
                    assert (out2[n:] == POISON).all(), what
                else:
                    assert (out2 == POISON).all(), what
                assert int(tot[0]) == (want_total if with_total else int(POISON)), what
                assert (tot[1:] == POISON).all(), what
        # the input is read, never written
        got_in = bufs["in"].to_array(np.uint32, cells)
        assert np.array_equal(got_in[:n], x) and (got_in[n:] == POISON).all(), name
