// gb_ewise_union.hip -- GxB_eWiseUnion: C<M> = accum(C, T), T on the structure of A' union B'.
//   GxB_{Matrix,Vector}_eWiseUnion   reference core/matrix.py:2044-2161, core/vector.py:1141-1260
//   T(i,j) = add(a, b) where both are stored, add(a, beta) where only A' is, add(alpha, b) where
//   only B' is; A', B', alpha and beta already have add's input type X, T its output type Z.
//
// Matrices: a merge of two CSRs done entry-parallel (a hub row of an R-MAT graph costs per entry
// what a row of 3 does, plus the logarithm of the other operand's row), no atomics, columns
// ascending, the same bits every run.  With S(q) = the number of B-only entries before entry q
// of B' (a scanned word base plus a popcount, as in gb_select.hip):
//   k_union_mark    entry q of B' is lane q & 63 of the wave that owns mark word q >> 6; its bit
//                   says "A' row i has no column bci[q]" (a binary search of that row).  The row
//                   of an entry comes from the wave row search of gb_select.hip.
//   gb_exclusive_scan_u8 over the words' popcounts: the bases of S, and S(nnz B') = the number
//                   of B-only entries (the one host read of the call: nvals(T) = nnz A' + that)
//   k_union_rowptr  orp[i] = arp[i] + S(brp[i]); brp[i] == nnz B' may name the word after the
//                   last: it exists and is zero
//   k_union_fill_a  entry p of A' (row i, column j), l = lower_bound(B' row i, j): it lands at
//                   orp[i] + (p - arp[i]) + S(l) - S(brp[i]) = p + S(l), with add(a, b) when
//                   bci[l] == j and add(a, beta) otherwise
//   k_union_fill_b  B-only entry q (row i, column j) lands at lower_bound(A' row i, j) + S(q)
//                   with add(alpha, b)
// Vectors (bitmap): k_union_vec, one lane per position, new word = ballot(a | b).
// The write-back (mask, replace, accum, cast to C's type) is gb_writeback_*, as for every
// operation.  "stat_union_both" / "_a_only" / "_b_only" hold the last call's entries per case.
#include <algorithm>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define UNI_BLOCK 256
#define UNI_WPI 4  // mark words (64 entries each) a wave handles per iteration
#define UNI_GRID_CAP 8192
#define UNI_VEC_GRID_CAP 1024  // blocks of the vector kernel, as for k_ewise_vec (gb_ops.hip)

namespace {

// S(q): the B-only entries before entry q of B' (q <= nnz B': that word exists)
GB_DEV int64_t uni_before(const uint64_t *__restrict__ words, const int64_t *__restrict__ base, int64_t q) {
    const int64_t w = q >> 6;
    return base[w] + __popcll(words[w] & ((1ull << (q & 63)) - 1));
}

// words [0, nw1): nw1 = bnz / 64 + 1 covers every entry of B' and leaves the last word's bits
// past bnz (or a whole last word, when bnz is a multiple of 64) zero.  A wave owns a contiguous
// run of chunks, so only its first chunk searches all of brp.
__global__ __launch_bounds__(UNI_BLOCK) void k_union_mark(int64_t nrows, int64_t bnz, int64_t nw1,
                                                          const int64_t *__restrict__ brp,
                                                          const int32_t *__restrict__ bci,
                                                          const int64_t *__restrict__ arp,
                                                          const int32_t *__restrict__ aci,
                                                          uint64_t *__restrict__ words, uint8_t *__restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * UNI_BLOCK) >> 6;
    const int64_t ngroups = (nw1 + UNI_WPI - 1) / UNI_WPI;
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)UNI_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t w0 = g * UNI_WPI;
        const int64_t p0 = w0 << 6;
        int64_t row[UNI_WPI];
        gb_chunk_rows<UNI_WPI>(brp, nrows, bnz, p0, lane, next, row);
        bool only[UNI_WPI];
#pragma unroll
        for (int u = 0; u < UNI_WPI; u++) {
            const int64_t q = p0 + u * 64 + lane;
            bool o = false;
            if (q < bnz) {
                const int32_t j = bci[q];
                const int64_t hi = arp[row[u] + 1];
                const int64_t l = gb_lower_bound(aci, arp[row[u]], hi, j);
                o = !(l < hi && aci[l] == j);
            }
            only[u] = o;
        }
#pragma unroll
        for (int u = 0; u < UNI_WPI; u++) {
            const unsigned long long b = __ballot(only[u]);
            if (lane == u && w0 + u < nw1) {
                words[w0 + u] = b;
                cnt[w0 + u] = (uint8_t)__popcll(b);
            }
        }
    }
}

__global__ __launch_bounds__(UNI_BLOCK) void k_union_rowptr(int64_t nrows, const int64_t *__restrict__ arp,
                                                            const int64_t *__restrict__ brp,
                                                            const uint64_t *__restrict__ words,
                                                            const int64_t *__restrict__ base,
                                                            int64_t *__restrict__ orp) {
    GB_GRID_LOOP(i, nrows + 1) { orp[i] = arp[i] + uni_before(words, base, brp[i]); }
}

template <class X, class Z>
__global__ __launch_bounds__(UNI_BLOCK) void k_union_fill_a(
    int64_t nrows, int64_t anz, int op, const int64_t *__restrict__ arp, const int32_t *__restrict__ aci,
    const X *__restrict__ ax, bool a_iso, const int64_t *__restrict__ brp, const int32_t *__restrict__ bci,
    const X *__restrict__ bx, bool b_iso, X beta, const uint64_t *__restrict__ words,
    const int64_t *__restrict__ base, int32_t *__restrict__ oci, Z *__restrict__ oz) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * UNI_BLOCK) >> 6;
    const int64_t ngroups = (anz + UNI_WPI * 64 - 1) / (UNI_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)UNI_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = (g * UNI_WPI) << 6;
        int64_t row[UNI_WPI];
        gb_chunk_rows<UNI_WPI>(arp, nrows, anz, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < UNI_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= anz) continue;
            const int64_t i = row[u];
            const int32_t j = aci[p];
            const int64_t hi = brp[i + 1];
            const int64_t l = gb_lower_bound(bci, brp[i], hi, j);
            const bool both = l < hi && bci[l] == j;
            X b = beta;
            if (both) b = bx[b_iso ? 0 : l];
            const int64_t dst = p + uni_before(words, base, l);
            oci[dst] = j;
            oz[dst] = gb_binop_z<X, Z>(op, ax[a_iso ? 0 : p], b, i, j, j);
        }
    }
}

// nw = ceil(bnz / 64): the words that can have a bit set
template <class X, class Z>
__global__ __launch_bounds__(UNI_BLOCK) void k_union_fill_b(
    int64_t nrows, int64_t bnz, int64_t nw, int op, const int64_t *__restrict__ brp,
    const int32_t *__restrict__ bci, const X *__restrict__ bx, bool b_iso, const int64_t *__restrict__ arp,
    const int32_t *__restrict__ aci, X alpha, const uint64_t *__restrict__ words,
    const int64_t *__restrict__ base, int32_t *__restrict__ oci, Z *__restrict__ oz) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t nwaves = ((int64_t)gridDim.x * UNI_BLOCK) >> 6;
    const int64_t ngroups = (nw + UNI_WPI - 1) / UNI_WPI;
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)UNI_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t w0 = g * UNI_WPI;
        const int64_t p0 = w0 << 6;
        unsigned long long word[UNI_WPI];
        unsigned long long any = 0;
#pragma unroll
        for (int u = 0; u < UNI_WPI; u++) {
            word[u] = w0 + u < nw ? words[w0 + u] : 0;
            any |= word[u];
        }
        if (!any) continue;  // the same in every lane; next stays a lower bound
        int64_t row[UNI_WPI];
        gb_chunk_rows<UNI_WPI>(brp, nrows, bnz, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < UNI_WPI; u++) {
            if (!((word[u] >> lane) & 1)) continue;  // a set bit is an entry below bnz (k_union_mark)
            const int64_t q = p0 + u * 64 + lane;
            const int64_t i = row[u];
            const int32_t j = bci[q];
            const int64_t la = gb_lower_bound(aci, arp[i], arp[i + 1], j);
            const int64_t dst = la + base[w0 + u] + __popcll(word[u] & below);
            oci[dst] = j;
            oz[dst] = gb_binop_z<X, Z>(op, alpha, bx[b_iso ? 0 : q], i, j, j);
        }
    }
}

// one lane per position; stat[0..3) += the positions with both, only u, only v
template <class X, class Z>
__global__ __launch_bounds__(UNI_BLOCK) void k_union_vec(int64_t n, int64_t nw, int op,
                                                         const uint64_t *__restrict__ ub, const X *__restrict__ ux,
                                                         bool u_iso, const uint64_t *__restrict__ vb,
                                                         const X *__restrict__ vx, bool v_iso, X alpha, X beta,
                                                         uint64_t *__restrict__ ob, Z *__restrict__ oz,
                                                         unsigned long long *__restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * UNI_BLOCK) >> 6;
    unsigned long long nboth = 0, na = 0, nb = 0;
    for (int64_t w = (blockIdx.x * (int64_t)UNI_BLOCK + threadIdx.x) >> 6; w < nw; w += nwaves) {
        const int64_t i = (w << 6) + lane;
        const bool a = i < n && ((ub[w] >> lane) & 1);
        const bool b = i < n && ((vb[w] >> lane) & 1);
        if (a || b) {
            X x = alpha, y = beta;
            if (a) x = ux[u_iso ? 0 : i];
            if (b) y = vx[v_iso ? 0 : i];
            oz[i] = gb_binop_z<X, Z>(op, x, y, i, 0, 0);
        }
        const unsigned long long wa = __ballot(a), wb = __ballot(b);
        if (lane == 0) {
            ob[w] = wa | wb;
            nboth += __popcll(wa & wb);
            na += __popcll(wa & ~wb);
            nb += __popcll(wb & ~wa);
        }
    }
    gb_block_add(nboth, stat);
    gb_block_add(na, stat + 1);
    gb_block_add(nb, stat + 2);
}

void uni_stats(int64_t both, int64_t a_only, int64_t b_only) {
    gb_stat_set("union_both", both);
    gb_stat_set("union_a_only", a_only);
    gb_stat_set("union_b_only", b_only);
}

// a vector call leaves its three counts here (device) until a reader asks
unsigned long long *g_vec_stat = nullptr;
bool g_vec_stat_pending = false;

template <class X>
X uni_scalar(const void *p) {
    X x;
    memcpy(&x, p, sizeof(X));
    return x;
}

void union_vector(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp add, GB_Obj *A, const void *alpha, GB_Obj *B,
                  const void *beta, const gb_desc &d) {
    const int64_t n = C->nrows;
    GB_REQUIRE(A->nrows == n && B->nrows == n && gb_ncols_of(A) == 1 && gb_ncols_of(B) == 1, GrB_DIMENSION_MISMATCH,
               "vector sizes do not match");
    const int xcode = add->xtype->code, zcode = add->ztype->code;
    gb_bitmap_view ua, ub;
    gb_get_bitmap(ua, A);
    gb_get_bitmap(ub, B);
    gb_scratch s;
    const void *xa = gb_bitmap_vals_as(ua, xcode, s), *xb = gb_bitmap_vals_as(ub, xcode, s);
    gb_vec_result T = gb_new_vec_result(n, zcode, false);
    const int64_t nw = gb_words(n);
    if (!g_vec_stat) g_vec_stat = gb_malloc_n<unsigned long long>(3);
    gb_memset(g_vec_stat, 0, 3 * sizeof(unsigned long long));
    g_vec_stat_pending = true;
    if (nw) {
        gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
            using X = decltype(x);
            using Z = decltype(z);
            hipLaunchKernelGGL((k_union_vec<X, Z>), dim3(gb_grid(nw, UNI_BLOCK / 64, UNI_VEC_GRID_CAP)), dim3(UNI_BLOCK),
                               0, gb_stream(), n, nw, add->opcode, ua.bits, (const X *)xa, ua.iso, ub.bits,
                               (const X *)xb, ub.iso, uni_scalar<X>(alpha), uni_scalar<X>(beta), T.bits, (Z *)T.dense,
                               g_vec_stat);
        });
        GB_LAUNCH_CHECK();
    }
    gb_bitmap_count(T.bits, T.n, T.d_nvals);
    gb_writeback_vector(C, T, M, d, accum, false);
}

void union_matrix(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp add, GB_Obj *A, const void *alpha, GB_Obj *B,
                  const void *beta, const gb_desc &d) {
    gb_csr_view av, bv;
    if (d.tran0) gb_get_csc(av, A);
    else gb_get_csr(av, A);
    if (d.tran1) gb_get_csc(bv, B);
    else gb_get_csr(bv, B);
    const int64_t nr = C->nrows, nc = C->ncols;
    GB_REQUIRE(av.nrows == nr && av.ncols == nc && bv.nrows == nr && bv.ncols == nc, GrB_DIMENSION_MISMATCH,
               "matrix dimensions do not match");
    const int xcode = add->xtype->code, zcode = add->ztype->code;
    gb_scratch s;
    const void *xa = gb_view_vals_as(av, xcode, s), *xb = gb_view_vals_as(bv, xcode, s);
    const int64_t anz = av.nvals, bnz = bv.nvals;
    gb_mat_result T;
    T.nrows = nr;
    T.ncols = nc;
    T.tcode = zcode;
    T.rowptr = gb_malloc_n<int64_t>(nr + 1);
    const int64_t nw1 = (bnz >> 6) + 1;
    uint64_t *words = s.get<uint64_t>(nw1);
    int64_t *base = s.get<int64_t>(nw1 + 1);
    int64_t b_only = 0;
    if (bnz) {
        uint8_t *cnt = s.get<uint8_t>(nw1);
        // a wave takes a run of chunks (4 or more, once there are that many)
        const unsigned grid = gb_grid(((nw1 + UNI_WPI - 1) / UNI_WPI + 3) / 4, UNI_BLOCK / 64, UNI_GRID_CAP);
        hipLaunchKernelGGL(k_union_mark, dim3(grid), dim3(UNI_BLOCK), 0, gb_stream(), nr, bnz, nw1, bv.rowptr,
                           bv.colidx, av.rowptr, av.colidx, words, cnt);
        GB_LAUNCH_CHECK();
        gb_exclusive_scan_u8(cnt, base, nw1);
        b_only = gb_read_i64(base + nw1);
    } else {
        gb_memset(words, 0, sizeof(uint64_t));
        gb_memset(base, 0, 2 * sizeof(int64_t));
    }
    const int64_t total = anz + b_only;
    T.nvals = total;
    T.colidx = gb_malloc_n<int32_t>(std::max<int64_t>(total, 1));
    T.vals = gb_malloc(std::max<int64_t>(total, 1) * gb_type_size(zcode));
    hipLaunchKernelGGL(k_union_rowptr, dim3(gb_grid((nr + 1 + 63) / 64, UNI_BLOCK / 64, UNI_GRID_CAP)),
                       dim3(UNI_BLOCK), 0, gb_stream(), nr, av.rowptr, bv.rowptr, words, base, T.rowptr);
    GB_LAUNCH_CHECK();
    gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
        using X = decltype(x);
        using Z = decltype(z);
        if (anz) {
            const unsigned grid =
                gb_grid(((gb_words(anz) + UNI_WPI - 1) / UNI_WPI + 3) / 4, UNI_BLOCK / 64, UNI_GRID_CAP);
            hipLaunchKernelGGL((k_union_fill_a<X, Z>), dim3(grid), dim3(UNI_BLOCK), 0, gb_stream(), nr, anz,
                               add->opcode, av.rowptr, av.colidx, (const X *)xa, av.iso, bv.rowptr, bv.colidx,
                               (const X *)xb, bv.iso, uni_scalar<X>(beta), words, base, T.colidx, (Z *)T.vals);
        }
        if (b_only) {
            const int64_t nw = gb_words(bnz);
            const unsigned grid = gb_grid(((nw + UNI_WPI - 1) / UNI_WPI + 3) / 4, UNI_BLOCK / 64, UNI_GRID_CAP);
            hipLaunchKernelGGL((k_union_fill_b<X, Z>), dim3(grid), dim3(UNI_BLOCK), 0, gb_stream(), nr, bnz, nw,
                               add->opcode, bv.rowptr, bv.colidx, (const X *)xb, bv.iso, av.rowptr, av.colidx,
                               uni_scalar<X>(alpha), words, base, T.colidx, (Z *)T.vals);
        }
    });
    GB_LAUNCH_CHECK();
    g_vec_stat_pending = false;
    uni_stats(bnz - b_only, anz - (bnz - b_only), b_only);
    gb_writeback_matrix(C, T, M, d, accum);
}

}  // namespace

void gb_union_stat_refresh(const char *key) {
    if (!g_vec_stat_pending || strncmp(key, "stat_union_", 11) != 0) return;
    unsigned long long h[3];
    gb_copy_d2h(h, g_vec_stat, sizeof(h));
    g_vec_stat_pending = false;
    uni_stats((int64_t)h[0], (int64_t)h[1], (int64_t)h[2]);
}

void gb_ewise_union(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp add, GB_Obj *A, const void *alpha,
                    GB_Obj *B, const void *beta, const gb_desc &d) {
    gb_check_binop(add, false);
    gb_check_binop(accum, true);
    GB_REQUIRE(add->xtype != nullptr, GrB_NOT_IMPLEMENTED, "positional eWiseUnion operator");
    if (C->kind != GB_KIND_MATRIX) union_vector(C, M, accum, add, A, alpha, B, beta, d);
    else union_matrix(C, M, accum, add, A, alpha, B, beta, d);
}
