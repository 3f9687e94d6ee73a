// taxscreen.hip — the taxonomy side of `taxscreen` for gfx950: one lowest-common-ancestor fold
// per entry of U over its holders (the loop of CommandTaxScreen.cpp:386-397 around
// TaxDB::getLowestCommonAncestor, taxdb.hpp:158-190), the per-taxon tallies (:398-403, minCov 1)
// and the clade sums up every tallied taxon's ancestors (:406-437).  The table (U, its
// counters, ustart / post) is screen's (screen.hip); the pool pass that fills the counters is
// screen_count_kernel in sketch.hip.
//
// The fold in closed form.  A state is one u32: kTaxNone (no holder with a taxon yet),
// kTaxUnknown (one holder whose taxID the dump lacks), a node, or kTaxTopped.  join(x, y) with
// both sides set is kTaxTopped when either is unknown or topped, when the two nodes share no
// ancestor, or when their deepest common ancestor is a root (the path of `a` stops before a
// root and before taxID 1, :176, and the walk from `b` stops at a root, :183: `return 1`);
// otherwise that ancestor.  join is commutative and associative, kTaxNone its identity and
// kTaxTopped absorbing, so the holders may be folded in any order and in parts.  kTaxTopped
// leaves the kernel as `top`, the node of taxID 1 (kTaxUnknown when the dump has none).
//
// Every walk up the tree is a counted loop over the depths the host computed while it checked
// the parent links for cycles: no loop here ends on a value read from the tree.
#include "fpm_kernels.hpp"

namespace fpm {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTaxTopped = 0xFFFFFFFDu;   // never leaves this file

// the deepest common ancestor of nodes a and b, kTaxTopped when they are in different trees
__device__ __forceinline__ uint32_t tax_common(const TaxTree &t, uint32_t a, uint32_t b)
{
    uint32_t da = t.depth[a], db = t.depth[b];
    for (; da > db && a < t.n_nodes; da--) a = t.parent[a];
    for (; db > da && b < t.n_nodes; db--) b = t.parent[b];
    for (; a != b && da > 0 && a < t.n_nodes && b < t.n_nodes; da--) {
        a = t.parent[a];
        b = t.parent[b];
    }
    return (a == b && a < t.n_nodes) ? a : kTaxTopped;
}

__device__ __forceinline__ uint32_t tax_join(const TaxTree &t, uint32_t x, uint32_t y)
{
    if (x == kTaxNone) return y;
    if (y == kTaxNone) return x;
    if (x >= t.n_nodes || y >= t.n_nodes) return kTaxTopped;   // unknown or topped
    const uint32_t c = tax_common(t, x, y);
    return (c == kTaxTopped || t.depth[c] == 0) ? kTaxTopped : c;
}

// One lane per entry of U for posting lists shorter than kTaxWaveCut; the longer lists of a
// wave's 64 entries are then folded one after the other by the whole wave, each lane over
// every 64th holder, the 64 partial states joined by a butterfly.  lca[u]: kTaxNone,
// kTaxUnknown or a node.  Tallies (CommandTaxScreen.cpp:398-403): tax_hashes[lca] += 1, and
// tax_count[lca] += 1 when the entry was seen in the pool; entries without a node only reach
// the totals.  totals[0] += entries seen in the pool; wave_entries += entries the wave folded.
__global__ __launch_bounds__(kThreads) void tax_lca_kernel(
    const uint32_t *__restrict__ count, const uint32_t *__restrict__ ustart,
    const uint32_t *__restrict__ post, uint32_t n, const uint32_t *__restrict__ ref_node,
    TaxTree t, uint32_t *__restrict__ lca, uint32_t *__restrict__ tax_hashes,
    uint32_t *__restrict__ tax_count, unsigned long long *__restrict__ totals,
    uint32_t *__restrict__ wave_entries)
{
    const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = u < n;
    uint32_t s = 0, e = 0;
    if (valid) {
        s = ustart[u];
        e = ustart[u + 1];
    }
    const bool wide = e - s >= kTaxWaveCut;
    uint32_t cur = kTaxNone;
    if (!wide)
        for (uint32_t p = s; p < e && cur != kTaxTopped; p++) cur = tax_join(t, cur, ref_node[post[p]]);
    unsigned long long todo = __ballot(wide);
    if (lane == 0 && todo) atomicAdd(wave_entries, (uint32_t)__popcll(todo));
    while (todo) {                                             // wave-uniform
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t js = __shfl(s, j, 64), je = __shfl(e, j, 64);
        uint32_t part = kTaxNone;
        for (uint32_t p = js + lane; p < je && part != kTaxTopped; p += 64)
            part = tax_join(t, part, ref_node[post[p]]);
        for (int o = 32; o; o >>= 1) {
            const uint32_t other = __shfl_xor(part, o, 64);
            part = tax_join(t, part, other);
        }
        if ((int)lane == j) cur = part;
    }
    if (cur == kTaxTopped) cur = t.top;
    const bool seen = valid && count[u] >= 1;
    if (valid) {
        lca[u] = cur;
        if (cur < t.n_nodes) {
            atomicAdd(&tax_hashes[cur], 1u);
            if (seen) atomicAdd(&tax_count[cur], 1u);
        }
    }
    const unsigned long long sb = __ballot(seen);
    if (lane == 0 && sb) atomicAdd(&totals[0], (unsigned long long)__popcll(sb));
}

// Clade sums (CommandTaxScreen.cpp:406-437): one lane per node; a node with a direct tally adds
// both tallies to itself and to each of its depth[v] ancestors, every taxon visited once.
__global__ __launch_bounds__(kThreads) void tax_clade_kernel(
    TaxTree t, const uint32_t *__restrict__ tax_hashes, const uint32_t *__restrict__ tax_count,
    uint32_t *__restrict__ clade_hashes, uint32_t *__restrict__ clade_count)
{
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t h = 0, c = 0, d = 0, x = v;
    if (v < t.n_nodes) {
        h = tax_hashes[v];                                     // c <= h
        c = tax_count[v];
        d = t.depth[v];
    }
    const bool live = h != 0;
    if (!__ballot(live)) return;                               // wave-uniform
    uint32_t deepest = live ? d : 0;
    for (int o = 32; o; o >>= 1) deepest = max(deepest, (uint32_t)__shfl_xor(deepest, o, 64));
    // The wave climbs level by level from its deepest tallied node; a lane joins at its own
    // depth, so the lanes stand on nodes of one level and meet in their common ancestors at the
    // same step.  Where they all stand on one node (the root and the taxa just below it, where
    // every path ends) the wave adds its sums once instead of 64 times to one address.
    for (uint32_t level = deepest + 1; level-- > 0;) {
        const bool on = live && d == level && x < t.n_nodes;
        const unsigned long long mask = __ballot(on);
        if (!mask) continue;
        const int first = __ffsll((long long)mask) - 1;
        const uint32_t x0 = __shfl(x, first, 64);
        if (__ballot(on && x == x0) == mask) {
            uint32_t hs = on ? h : 0, cs = on ? c : 0;
            for (int o = 32; o; o >>= 1) {
                hs += __shfl_xor(hs, o, 64);
                cs += __shfl_xor(cs, o, 64);
            }
            if ((int)lane == first) {
                atomicAdd(&clade_hashes[x0], hs);
                if (cs) atomicAdd(&clade_count[x0], cs);
            }
        } else if (on) {
            atomicAdd(&clade_hashes[x], h);
            if (c) atomicAdd(&clade_count[x], c);
        }
        if (on) {
            x = t.parent[x];
            d--;                                               // wraps past a root: never on again
        }
    }
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kThreads - 1) / kThreads)); }

}  // namespace

hipError_t launch_tax_lca(const uint32_t *d_count, const uint32_t *d_ustart, const uint32_t *d_post,
                          uint32_t n, const uint32_t *d_ref_node, const TaxTree &t, uint32_t *d_lca,
                          uint32_t *d_tax_hashes, uint32_t *d_tax_count,
                          unsigned long long *d_totals, uint32_t *d_wave_entries, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(tax_lca_kernel, grid_for(n), dim3(kThreads), 0, st, d_count, d_ustart,
                       d_post, n, d_ref_node, t, d_lca, d_tax_hashes, d_tax_count, d_totals,
                       d_wave_entries);
    return hipGetLastError();
}

hipError_t launch_tax_clade(const TaxTree &t, const uint32_t *d_tax_hashes,
                            const uint32_t *d_tax_count, uint32_t *d_clade_hashes,
                            uint32_t *d_clade_count, hipStream_t st)
{
    if (!t.n_nodes) return hipSuccess;
    hipLaunchKernelGGL(tax_clade_kernel, grid_for(t.n_nodes), dim3(kThreads), 0, st, t,
                       d_tax_hashes, d_tax_count, d_clade_hashes, d_clade_count);
    return hipGetLastError();
}

}  // namespace fpm
