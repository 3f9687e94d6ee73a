// fpm_contain_api.cpp — the contain part of the C ABI (include/fpmash.h): the (common, steps)
// grid of containSketches (CommandContain.cpp:314-412) on device or host rows.  The kernels
// are in contain.hip; which one runs is decided here from the rows' order, read back from the
// device, and from the context's contain mode.
#include "fpm_internal.hpp"

namespace {

int contain_impl(fpm_ctx *ctx, const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                 uint32_t *d_common, uint32_t *d_steps, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    ctx->last_contain_kernel = FPM_CK_NONE;
    if ((uint64_t)R.n * Q.n == 0) return FPM_OK;
    if (!R.rows || !R.len || !Q.rows || !Q.len || !d_common || !d_steps)
        return fail(FPM_EINVAL, "fpm_contain: null buffer");
    hipStream_t st = pick_stream(ctx, stream);
    bool literal = ctx->contain_mode == FPM_CONTAIN_LITERAL;
    uint32_t max_qry_len = 0;
    if (!literal) {
        void *ctr;
        HIP_TRY(scratch(ctx, kSlotCounters, kCtrWords * 8, &ctr));
        uint32_t *flag = (uint32_t *)((unsigned long long *)ctr + kCtrContain);
        HIP_TRY(hipMemsetAsync(flag, 0, 8, st));
        HIP_TRY(launch_rows_ascending(R, Q, hash_bytes, flag, st));
        uint32_t host[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(host, flag, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        literal = host[0] != 0;
        max_qry_len = host[1];
    }
    TimedLaunch tl(ctx, FPM_K_COMPARE, st);
    if (literal) {
        HIP_TRY(launch_contain_literal(R, Q, hash_bytes, d_common, d_steps, st));
        ctx->last_contain_kernel = FPM_CK_LITERAL;
    } else {
        bool lds = false;
        HIP_TRY(launch_contain_rows(R, Q, hash_bytes, max_qry_len, d_common, d_steps, &lds, st));
        ctx->last_contain_kernel = lds ? FPM_CK_ROWS_LDS : FPM_CK_ROWS_GLOBAL;
    }
    tl.done();
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_contain_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                    uint64_t ref_stride, uint32_t n_ref, const void *d_qry,
                    const uint32_t *d_qry_len, uint64_t qry_stride, uint32_t n_qry,
                    uint32_t hash_bytes, uint32_t *d_common, uint32_t *d_steps, void *stream)
{
    return contain_impl(ctx, RowSet{d_ref, d_ref_len, nullptr, ref_stride, n_ref},
                        RowSet{d_qry, d_qry_len, nullptr, qry_stride, n_qry}, hash_bytes, d_common,
                        d_steps, stream);
}

int fpm_contain(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len, uint64_t ref_stride,
                uint32_t n_ref, const void *qry, const uint32_t *qry_len, uint64_t qry_stride,
                uint32_t n_qry, uint32_t hash_bytes, uint32_t *out_common, uint32_t *out_steps)
{
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    const uint64_t np = (uint64_t)n_ref * n_qry;
    if (np == 0) {
        ctx->last_contain_kernel = FPM_CK_NONE;
        return FPM_OK;
    }
    if (!ref || !ref_len || !qry || !qry_len || !out_common || !out_steps)
        return fail(FPM_EINVAL, "fpm_contain: null buffer");
    // one set against itself: one upload
    const bool same = ref == qry && ref_len == qry_len && ref_stride == qry_stride && n_ref == n_qry;
    DevBufs mem(ctx);
    void *r, *q = nullptr;
    uint32_t *rl, *ql = nullptr, *co, *stp;
    hipError_t e = mem.upload(ctx, &r, ref, (size_t)n_ref * ref_stride * hash_bytes);
    if (e == hipSuccess) e = mem.upload(ctx, &rl, ref_len, (size_t)n_ref * 4);
    if (e == hipSuccess && !same) e = mem.upload(ctx, &q, qry, (size_t)n_qry * qry_stride * hash_bytes);
    if (e == hipSuccess && !same) e = mem.upload(ctx, &ql, qry_len, (size_t)n_qry * 4);
    if (e == hipSuccess) e = mem.get(&co, np * 4);
    if (e == hipSuccess) e = mem.get(&stp, np * 4);
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("contain staging: ") + hipGetErrorString(e));
    if (int rc = contain_impl(ctx, RowSet{r, rl, nullptr, ref_stride, n_ref},
                              RowSet{same ? r : q, same ? rl : ql, nullptr, qry_stride, n_qry},
                              hash_bytes, co, stp, nullptr))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(copy_out(ctx, out_common, co, np * 4));
    HIP_TRY(copy_out(ctx, out_steps, stp, np * 4));
    return FPM_OK;
}

int fpm_ctx_set_contain_mode(fpm_ctx *ctx, int mode)
{
    if (!ctx || (mode != FPM_CONTAIN_AUTO && mode != FPM_CONTAIN_LITERAL))
        return fail(FPM_EINVAL, "bad contain mode");
    ctx->contain_mode = mode;
    return FPM_OK;
}

int fpm_ctx_last_contain_kernel(fpm_ctx *ctx, int *kernel)
{
    if (!ctx || !kernel) return fail(FPM_EINVAL, "null argument");
    *kernel = ctx->last_contain_kernel;
    return FPM_OK;
}

int fpm_contain_lds_cap(fpm_ctx *ctx, uint32_t hash_bytes, uint32_t *cap)
{
    if (!cap) return fail(FPM_EINVAL, "null argument");
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    *cap = contain_lds_cap(hash_bytes);
    return FPM_OK;
}

}  // extern "C"
