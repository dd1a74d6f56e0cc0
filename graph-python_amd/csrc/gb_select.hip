// gb_select.hip -- GrB_select: C<M> = accum(C, the entries of A' an index-unary operator keeps).
//   GrB_{Matrix,Vector}_select_<T>   reference core/matrix.py:2452-2551, core/vector.py:1463-1560
//
// A structure-changing stream compaction, entry-parallel on wave64 ballots (a hub row of an
// R-MAT graph costs per entry what a row of 3 does), no atomics, output in input order:
//   k_select_mark     entry p is lane p & 63 of the wave that owns keep word p >> 6 (bit b of
//                     word w is entry 64 w + b); the ballot of the predicate is the word, its
//                     popcount one byte.  Positional operators never read the values, value
//                     operators never need the row.  The row of entry p is
//                     upper_bound(rowptr, p) - 1 (which skips runs of empty rows): the wave
//                     finds the bound of its chunk's first and last entry, then each lane
//                     looks inside that range only -- no row-of-entry array exists.
//   gb_exclusive_scan_u8 over the bytes: the first output position of every word, and the total
//                     (the one host read of the call: it sizes T)
//   k_select_scatter  a kept entry goes to base[w] + popc(word & lanes below)
//   k_select_rowptr   new_rowptr[i] = base[rowptr[i] >> 6] + popc(word & bits below rowptr[i] & 63);
//                     rowptr[i] == nvals may name the word after the last: it exists and is zero
// Vectors (bitmap): k_select_vec, one lane per position, new word = ballot(bit & predicate);
// the dense values are copied as they are.
// The operators themselves are gb_indexop.cuh's, shared with gb_apply_index.hip; an index-valued one
// (ROWINDEX, COLINDEX, DIAGINDEX) keeps the entries whose result is not zero.
// T has A's type and values (the operator's type serves the comparison only); the write-back
// (mask, replace, accum, cast to C's type) is gb_writeback_*, as for every operation.
#include <algorithm>

#include "gb_indexop.cuh"
#include "gb_internal.h"

#define SEL_BLOCK 256
#define SEL_WPI 4  // keep words (64 entries each) a wave handles per iteration
#define SEL_GRID_CAP 8192

namespace {

enum { SEL_ROWCOL = 0, SEL_COL = 1, SEL_VALUE = 2 };

// words [0, nw1): nw1 = nvals / 64 + 1 covers every entry and leaves the last word's bits past
// nvals (or a whole last word, when nvals is a multiple of 64) zero.  A wave owns a contiguous
// run of chunks (SEL_WPI words each), so only its first chunk searches all of rowptr: the rows
// of the next chunk start where the last one's ended.  Inside a chunk the row boundaries
// rowptr[rlo .. rhi) sit one per lane (relative to the chunk's first entry, at most 64 of them
// -- else every lane searches [rlo, rhi] itself), and an entry's row is rlo - 1 + the number of
// boundaries at or below it, counted with one readlane per boundary.
template <int MODE, class X>
__global__ __launch_bounds__(SEL_BLOCK) void k_select_mark(int64_t nvals, int64_t nrows, int64_t nw1, int op,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ colidx,
                                                           const X *__restrict__ vals, bool iso, int64_t k, X y,
                                                           uint64_t *__restrict__ words, uint8_t *__restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * SEL_BLOCK) >> 6;
    const int64_t ngroups = (nw1 + SEL_WPI - 1) / SEL_WPI;
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)SEL_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    X xiso = X();
    if (MODE == SEL_VALUE && iso && nvals) xiso = vals[0];
    int64_t next = -1;  // a lower bound of the next chunk's rlo (-1: not known yet)
    for (int64_t g = g0; g < g1; g++) {
        const int64_t w0 = g * SEL_WPI;
        const int64_t p0 = w0 << 6;
        int64_t rlo = 0, rhi = 0;
        int nb = -1;         // boundaries held one per lane in rel (-1: search per lane)
        int rel = INT32_MAX;  // rowptr[rlo + lane] - p0 for lane < nb
        if (MODE == SEL_ROWCOL && p0 < nvals) {
            const int64_t plast = min(p0 + SEL_WPI * 64, nvals) - 1;
            int64_t mine;
            rlo = next < 0 ? gb_upper_bound(rowptr, 1, nrows, p0) : gb_wave_upper(rowptr, next, nrows, p0, lane, &mine);
            rhi = gb_wave_upper(rowptr, rlo, nrows, plast, lane, &mine);
            next = rhi;
            if (rhi - rlo < 64) {
                nb = (int)(rhi - rlo);
                if (lane < nb) rel = (int)(mine - p0);  // in [1, SEL_WPI * 64)
            }
        }
        int below[SEL_WPI];
        gb_count_bounds<SEL_WPI>(rel, 0, nb, lane, below);
        bool keep[SEL_WPI];
#pragma unroll
        for (int u = 0; u < SEL_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            bool kp = false;
            if (p < nvals) {
                if (MODE == SEL_VALUE) {
                    kp = gb_iop_value<X>(op, iso ? xiso : vals[p], y);
                } else {
                    const int64_t j = colidx[p];
                    int64_t i = 0;
                    if (MODE == SEL_ROWCOL) i = (nb >= 0 ? rlo + below[u] : gb_upper_bound(rowptr, rlo, rhi, p)) - 1;
                    kp = gb_iop_positional(op, i, j, k, (int64_t)y);
                }
            }
            keep[u] = kp;
        }
#pragma unroll
        for (int u = 0; u < SEL_WPI; u++) {
            const unsigned long long b = __ballot(keep[u]);
            if (lane == u && w0 + u < nw1) {
                words[w0 + u] = b;
                cnt[w0 + u] = (uint8_t)__popcll(b);
            }
        }
    }
}

// VS: bytes per value, 0 = no values to move (iso)
template <int VS>
__global__ __launch_bounds__(SEL_BLOCK) void k_select_scatter(int64_t nw, const uint64_t *__restrict__ words,
                                                              const int64_t *__restrict__ base,
                                                              const int32_t *__restrict__ colidx,
                                                              const void *__restrict__ vals_,
                                                              int32_t *__restrict__ ocol, void *__restrict__ ovals_) {
    using V = gb_word_t<VS>;
    const V *__restrict__ vals = (const V *)vals_;
    V *__restrict__ ovals = (V *)ovals_;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t nwaves = ((int64_t)gridDim.x * SEL_BLOCK) >> 6;
    const int64_t ngroups = (nw + SEL_WPI - 1) / SEL_WPI;
    for (int64_t g = (blockIdx.x * (int64_t)SEL_BLOCK + threadIdx.x) >> 6; g < ngroups; g += nwaves) {
        const int64_t w0 = g * SEL_WPI;
#pragma unroll
        for (int u = 0; u < SEL_WPI; u++) {
            const int64_t w = w0 + u;
            if (w >= nw) break;
            const unsigned long long word = words[w];
            if (!((word >> lane) & 1)) continue;  // a set bit is an entry below nvals (k_select_mark)
            const int64_t p = (w << 6) + lane;
            const int64_t dst = base[w] + __popcll(word & below);
            ocol[dst] = colidx[p];
            if (VS) ovals[dst] = vals[p];
        }
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_select_rowptr(int64_t nrows, const int64_t *__restrict__ rowptr,
                                                             const uint64_t *__restrict__ words,
                                                             const int64_t *__restrict__ base,
                                                             int64_t *__restrict__ orowptr) {
    GB_GRID_LOOP(i, nrows + 1) {
        const int64_t r = rowptr[i];
        const int64_t w = r >> 6;  // at most nvals >> 6: the word after the last exists and is zero
        orowptr[i] = base[w] + __popcll(words[w] & ((1ull << (r & 63)) - 1));
    }
}

// one lane per position; positional operators see (i, 0)
template <bool VALUE, class X>
__global__ __launch_bounds__(SEL_BLOCK) void k_select_vec(int64_t n, int64_t nw, int op,
                                                          const uint64_t *__restrict__ bits,
                                                          const X *__restrict__ vals, bool iso, int64_t k, X y,
                                                          uint64_t *__restrict__ obits) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * SEL_BLOCK) >> 6;
    for (int64_t w = (blockIdx.x * (int64_t)SEL_BLOCK + threadIdx.x) >> 6; w < nw; w += nwaves) {
        const int64_t i = (w << 6) + lane;
        bool kp = false;
        if (i < n && ((bits[w] >> lane) & 1)) {
            if (VALUE) kp = gb_iop_value<X>(op, vals[iso ? 0 : i], y);
            else kp = gb_iop_positional(op, i, 0, k, (int64_t)y);
        }
        const unsigned long long b = __ballot(kp);
        if (lane == 0) obits[w] = b;
    }
}

void select_vector(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
                   const gb_desc &d) {
    GB_REQUIRE(A->nrows == C->nrows && (A->kind != GB_KIND_MATRIX || A->ncols == 1), GrB_DIMENSION_MISMATCH,
               "vector sizes do not match");
    gb_bitmap_view uv;
    gb_get_bitmap(uv, A);
    const size_t vs = gb_type_size(uv.tcode);
    const int64_t nw = gb_words(uv.n);
    gb_vec_result T = gb_new_vec_result(uv.n, uv.tcode, uv.iso);
    const int64_t nv = uv.iso ? 1 : uv.n;
    if (nw) {
        const unsigned grid = gb_grid(nw, SEL_BLOCK / 64, SEL_GRID_CAP);
        if (op->xtype) {
            gb_scratch s;
            const void *xin = gb_bitmap_vals_as(uv, op->xtype->code, s);
            gb_with_type(op->xtype->code, [&](auto xv) {
                using X = decltype(xv);
                hipLaunchKernelGGL((k_select_vec<true, X>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(), uv.n, nw,
                                   op->opcode, uv.bits, (const X *)xin, uv.iso, (int64_t)0,
                                   gb_iop_thunk<X>(y, ycode, op->xtype->code), T.bits);
            });
        } else {
            // a positional launch has no value thunk: its y carries the bits of an index-valued result
            int64_t zmask;
            const int64_t k = gb_iop_thunk_pos(op->opcode, y, ycode, op->ytype->code, &zmask);
            hipLaunchKernelGGL((k_select_vec<false, int64_t>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(), uv.n, nw,
                               op->opcode, uv.bits, (const int64_t *)nullptr, false, k, zmask, T.bits);
        }
        GB_LAUNCH_CHECK();
        gb_copy_d2d(T.dense, uv.vals, nv * vs);
    }
    gb_bitmap_count(T.bits, T.n, T.d_nvals);
    gb_writeback_vector(C, T, M, d, accum, false);
}

void select_matrix(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
                   const gb_desc &d) {
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    GB_REQUIRE(v.nrows == C->nrows && v.ncols == C->ncols, GrB_DIMENSION_MISMATCH, "matrix dimensions do not match");
    const size_t vs = gb_type_size(v.tcode);
    gb_mat_result T;
    T.nrows = v.nrows;
    T.ncols = v.ncols;
    T.tcode = v.tcode;
    T.iso = v.iso;
    T.rowptr = gb_malloc_n<int64_t>(v.nrows + 1);
    int64_t total = 0;
    gb_scratch s;
    uint64_t *words = nullptr;
    int64_t *base = nullptr;
    const int64_t nw1 = (v.nvals >> 6) + 1;
    if (v.nvals) {
        words = s.get<uint64_t>(nw1);
        uint8_t *cnt = s.get<uint8_t>(nw1);
        base = s.get<int64_t>(nw1 + 1);
        // a wave takes a run of chunks (4 or more, once there are that many)
        const unsigned grid = gb_grid(((nw1 + SEL_WPI - 1) / SEL_WPI + 3) / 4, SEL_BLOCK / 64, SEL_GRID_CAP);
        if (op->xtype) {
            const void *xin = gb_view_vals_as(v, op->xtype->code, s);
            gb_with_type(op->xtype->code, [&](auto xv) {
                using X = decltype(xv);
                hipLaunchKernelGGL((k_select_mark<SEL_VALUE, X>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(),
                                   v.nvals, v.nrows, nw1, op->opcode, v.rowptr, v.colidx, (const X *)xin, v.iso,
                                   (int64_t)0, gb_iop_thunk<X>(y, ycode, op->xtype->code), words, cnt);
            });
        } else {
            // a positional launch has no value thunk: its y carries the bits of an index-valued result
            int64_t zmask;
            const int o = op->opcode;
            const int64_t k = gb_iop_thunk_pos(o, y, ycode, op->ytype->code, &zmask);
            if (gb_iop_needs_row(o))
                hipLaunchKernelGGL((k_select_mark<SEL_ROWCOL, int64_t>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(),
                                   v.nvals, v.nrows, nw1, o, v.rowptr, v.colidx, (const int64_t *)nullptr, false, k,
                                   zmask, words, cnt);
            else
                hipLaunchKernelGGL((k_select_mark<SEL_COL, int64_t>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(),
                                   v.nvals, v.nrows, nw1, o, v.rowptr, v.colidx, (const int64_t *)nullptr, false, k,
                                   zmask, words, cnt);
        }
        GB_LAUNCH_CHECK();
        gb_exclusive_scan_u8(cnt, base, nw1);
        total = gb_read_i64(base + nw1);
    }
    T.nvals = total;
    T.colidx = gb_malloc_n<int32_t>(std::max<int64_t>(total, 1));
    const int64_t nv = v.iso ? (total ? 1 : 0) : total;
    T.vals = gb_malloc(std::max<int64_t>(nv, 1) * vs);
    if (total == 0) {
        gb_memset(T.rowptr, 0, (v.nrows + 1) * sizeof(int64_t));
    } else if (total == v.nvals) {
        // everything kept: copies, so that C may be A
        gb_copy_d2d(T.rowptr, v.rowptr, (v.nrows + 1) * sizeof(int64_t));
        gb_copy_d2d(T.colidx, v.colidx, total * sizeof(int32_t));
        gb_copy_d2d(T.vals, v.vals, nv * vs);
    } else {
        const int64_t nw = gb_words(v.nvals);
        const unsigned grid = gb_grid((nw + SEL_WPI - 1) / SEL_WPI, SEL_BLOCK / 64, SEL_GRID_CAP);
        auto scatter = [&](auto vsize) {
            hipLaunchKernelGGL((k_select_scatter<decltype(vsize)::value>), dim3(grid), dim3(SEL_BLOCK), 0, gb_stream(),
                               nw, words, base, v.colidx, v.vals, T.colidx, T.vals);
        };
        if (v.iso) scatter(std::integral_constant<int, 0>{});
        else gb_with_size(vs, [&](auto w) { scatter(std::integral_constant<int, (int)sizeof(w)>{}); });
        GB_LAUNCH_CHECK();
        if (v.iso) gb_copy_d2d(T.vals, v.vals, vs);
        hipLaunchKernelGGL(k_select_rowptr, dim3(gb_grid((v.nrows + 1 + 63) / 64, SEL_BLOCK / 64, SEL_GRID_CAP)),
                           dim3(SEL_BLOCK), 0, gb_stream(), v.nrows, v.rowptr, words, base, T.rowptr);
        GB_LAUNCH_CHECK();
    }
    gb_writeback_matrix(C, T, M, d, accum);
}

}  // namespace

void gb_select(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
               const gb_desc &d) {
    GB_REQUIRE(op, GrB_NULL_POINTER, "operator is NULL");
    GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid operator");
    gb_check_binop(accum, true);
    GB_REQUIRE(op->opcode >= 0 && op->opcode < GBAMD_IOP_COUNT, GrB_INVALID_VALUE, "unknown index-unary operator");
    if (C->kind != GB_KIND_MATRIX) select_vector(C, M, accum, op, A, y, ycode, d);
    else select_matrix(C, M, accum, op, A, y, ycode, d);
}

extern "C" {

#define GB_DEFINE_SELECT(T, ctype)                                                                            \
    GrB_Info GrB_Matrix_select_##T(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,             \
                                   const GrB_IndexUnaryOp op, const GrB_Matrix A, ctype y,                    \
                                   const GrB_Descriptor desc) {                                               \
        return gb_api(OBJ(C), [&] {                                                                           \
            gb_select(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), &y, GBAMD_T_##T, \
                      gb_read_desc(desc));                                                                    \
        });                                                                                                   \
    }                                                                                                         \
    GrB_Info GrB_Vector_select_##T(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,             \
                                   const GrB_IndexUnaryOp op, const GrB_Vector u, ctype y,                    \
                                   const GrB_Descriptor desc) {                                               \
        return gb_api(OBJ(w), [&] {                                                                           \
            gb_select(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(u), &y, GBAMD_T_##T, \
                      gb_read_desc(desc));                                                                    \
        });                                                                                                   \
    }

GB_FOR_EACH_TYPE(GB_DEFINE_SELECT)

}  // extern "C"
