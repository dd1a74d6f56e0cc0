// gb_apply_index.hip -- GrB_apply with an index-unary operator:
// C<M> = accum(C, f(A'(i, j), i, j, y)).
//   GrB_{Matrix,Vector}_apply_IndexOp_<T>   reference core/matrix.py:2337-2437, core/vector.py (same method)
//
// T has exactly the structure of A': every stored entry yields a stored result, a 0 or a false
// included.  ROWINDEX / COLINDEX / DIAGINDEX store i + y, j + y, j - i + y in the operator's type
// (INT32 or INT64; computed in 64 bits, then cast as C casts); the select operators (TRIL .. ROWGT,
// VALUE*_<T>) store their predicate as BOOL.  The operators are gb_indexop.cuh's, the ones
// gb_select.hip filters with.
//   k_apply_index      entry-parallel: entry p is lane p & 63 of a wave step, IDX_WPI steps to a
//                      chunk, so a hub row of an R-MAT graph costs per entry what a row of 3 does.
//                      A wave owns a contiguous run of chunks; the rows of a chunk's entries are
//                      gb_chunk_rows' (one search of rowptr for the wave's first chunk, the bound
//                      carried to the next, a per-lane search when a chunk holds 64 or more row
//                      boundaries): no row-of-entry array exists.  The column operators read
//                      colidx only and the value operators the values only; a positional operator
//                      never reads, casts or copies the values.
//   k_apply_index_vec  vectors (bitmap): one lane per position, entry (i, 0); the bit words are
//                      copied, the dense result is written where there is an entry.
// rowptr and colidx of T are device copies of the view's, so C may be A.  An iso input gives an
// iso BOOL result under a value operator (one evaluation) and a non-iso result under a positional
// one.  The write-back (mask, replace, accum, cast to C's type) is gb_writeback_*, as for every
// operation.
#include "gb_indexop.cuh"
#include "gb_internal.h"

#define IDX_BLOCK 256
#define IDX_WPI 4  // wave steps (64 entries each) to a chunk
#define IDX_GRID_CAP 8192

namespace {

enum { IDX_ROWCOL = 0, IDX_COL = 1, IDX_VALUE = 2 };

// z of one entry: Z = bool for the predicates, int32_t / int64_t for the index-valued operators
template <class Z>
GB_DEV Z idx_positional(int op, int64_t i, int64_t j, int64_t k) {
    if constexpr (std::is_same<Z, bool>::value) return gb_iop_positional(op, i, j, k, -1);
    else return (Z)gb_iop_index(op, i, j, k);
}

// out[p] = z of entry p, p in [0, nvals).  IDX_VALUE: z = gb_iop_value(vals[p], y), X the
// operator's type; else X is unused and z comes from (row, colidx[p], k).
template <int MODE, class X, class Z>
__global__ __launch_bounds__(IDX_BLOCK) void k_apply_index(int64_t nvals, int64_t nrows, int op,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ colidx,
                                                           const X *__restrict__ vals, int64_t k, X y,
                                                           Z *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * IDX_BLOCK) >> 6;
    const int64_t ngroups = (nvals + IDX_WPI * 64 - 1) / (IDX_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)IDX_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;  // where the row search of the wave's previous chunk ended
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * (IDX_WPI * 64);
        int64_t row[IDX_WPI];
        if (MODE == IDX_ROWCOL) gb_chunk_rows<IDX_WPI>(rowptr, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < IDX_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= nvals) continue;
            if (MODE == IDX_VALUE) out[p] = (Z)gb_iop_value<X>(op, vals[p], y);
            else out[p] = idx_positional<Z>(op, MODE == IDX_ROWCOL ? row[u] : 0, colidx[p], k);
        }
    }
}

// one lane per position; a positional operator sees (i, 0)
template <bool VALUE, class X, class Z>
__global__ __launch_bounds__(IDX_BLOCK) void k_apply_index_vec(int64_t n, int64_t nw, int op,
                                                               const uint64_t *__restrict__ bits,
                                                               const X *__restrict__ vals, int64_t k, X y,
                                                               uint64_t *__restrict__ obits, Z *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * IDX_BLOCK) >> 6;
    for (int64_t w = (blockIdx.x * (int64_t)IDX_BLOCK + threadIdx.x) >> 6; w < nw; w += nwaves) {
        const uint64_t word = bits[w];
        if (lane == 0) obits[w] = word;
        const int64_t i = (w << 6) + lane;
        if (i >= n || !((word >> lane) & 1)) continue;
        if (VALUE) out[i] = (Z)gb_iop_value<X>(op, vals[i], y);
        else out[i] = idx_positional<Z>(op, i, 0, k);
    }
}

// f(Z{}) for the result type of a positional operator
template <class F>
void with_ztype(int zcode, F &&f) {
    if (zcode == GBAMD_T_BOOL) f(bool{});
    else if (zcode == GBAMD_T_INT32) f(int32_t{});
    else f(int64_t{});
}

// the one evaluation of a value operator on an iso input: out[0] = f(vals[0], y)
void value_once(GrB_IndexUnaryOp op, const void *xin, const void *y, int ycode, void *out) {
    gb_with_type(op->xtype->code, [&](auto xv) {
        using X = decltype(xv);
        hipLaunchKernelGGL((k_apply_index<IDX_VALUE, X, bool>), dim3(1), dim3(IDX_BLOCK), 0, gb_stream(), (int64_t)1,
                           (int64_t)0, op->opcode, (const int64_t *)nullptr, (const int32_t *)nullptr, (const X *)xin,
                           (int64_t)0, gb_iop_thunk<X>(y, ycode, op->xtype->code), (bool *)out);
    });
    GB_LAUNCH_CHECK();
}

void apply_index_vector(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, int zcode, GB_Obj *A,
                        const void *y, int ycode, const gb_desc &d) {
    GB_REQUIRE(A->nrows == C->nrows && (A->kind != GB_KIND_MATRIX || A->ncols == 1), GrB_DIMENSION_MISMATCH,
               "vector sizes do not match");
    gb_bitmap_view uv;
    gb_get_bitmap(uv, A);
    const int64_t nw = gb_words(uv.n);
    const bool iso = op->xtype && uv.iso;
    gb_vec_result T = gb_new_vec_result(uv.n, zcode, iso);
    gb_scratch s;
    if (iso && nw) {
        gb_copy_d2d(T.bits, uv.bits, nw * sizeof(uint64_t));
        value_once(op, gb_bitmap_vals_as(uv, op->xtype->code, s), y, ycode, T.dense);
    } else if (nw) {
        const unsigned grid = gb_grid(nw, IDX_BLOCK / 64, IDX_GRID_CAP);
        if (op->xtype) {
            const void *xin = gb_bitmap_vals_as(uv, op->xtype->code, s);
            gb_with_type(op->xtype->code, [&](auto xv) {
                using X = decltype(xv);
                hipLaunchKernelGGL((k_apply_index_vec<true, X, bool>), dim3(grid), dim3(IDX_BLOCK), 0, gb_stream(),
                                   uv.n, nw, op->opcode, uv.bits, (const X *)xin, (int64_t)0,
                                   gb_iop_thunk<X>(y, ycode, op->xtype->code), T.bits, (bool *)T.dense);
            });
        } else {
            int64_t zmask;
            const int64_t k = gb_iop_thunk_pos(op->opcode, y, ycode, op->ytype->code, &zmask);
            with_ztype(zcode, [&](auto zv) {
                using Z = decltype(zv);
                hipLaunchKernelGGL((k_apply_index_vec<false, int64_t, Z>), dim3(grid), dim3(IDX_BLOCK), 0, gb_stream(),
                                   uv.n, nw, op->opcode, uv.bits, (const int64_t *)nullptr, k, (int64_t)0, T.bits,
                                   (Z *)T.dense);
            });
        }
        GB_LAUNCH_CHECK();
    }
    if (uv.count) gb_copy_d2d(T.d_nvals, uv.count, sizeof(int64_t));
    else gb_bitmap_count(T.bits, T.n, T.d_nvals);
    gb_writeback_vector(C, T, M, d, accum, false);
}

void apply_index_matrix(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, int zcode, GB_Obj *A,
                        const void *y, int ycode, const gb_desc &d) {
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    GB_REQUIRE(v.nrows == C->nrows && v.ncols == C->ncols, GrB_DIMENSION_MISMATCH, "matrix dimensions do not match");
    const bool iso = op->xtype && v.iso;
    gb_mat_result T = gb_new_mat_result(v.nrows, v.ncols, zcode, v.nvals, iso);
    // copies, so that C may be A
    gb_copy_d2d(T.rowptr, v.rowptr, (v.nrows + 1) * sizeof(int64_t));
    if (v.nvals) gb_copy_d2d(T.colidx, v.colidx, v.nvals * sizeof(int32_t));
    gb_scratch s;
    if (iso) {
        if (v.nvals) value_once(op, gb_view_vals_as(v, op->xtype->code, s), y, ycode, T.vals);
    } else if (v.nvals) {
        // a wave takes a run of chunks (4 or more, once there are that many)
        const int64_t ngroups = (v.nvals + IDX_WPI * 64 - 1) / (IDX_WPI * 64);
        const unsigned grid = gb_grid((ngroups + 3) / 4, IDX_BLOCK / 64, IDX_GRID_CAP);
        if (op->xtype) {
            const void *xin = gb_view_vals_as(v, op->xtype->code, s);
            gb_with_type(op->xtype->code, [&](auto xv) {
                using X = decltype(xv);
                hipLaunchKernelGGL((k_apply_index<IDX_VALUE, X, bool>), dim3(grid), dim3(IDX_BLOCK), 0, gb_stream(),
                                   v.nvals, v.nrows, op->opcode, v.rowptr, v.colidx, (const X *)xin, (int64_t)0,
                                   gb_iop_thunk<X>(y, ycode, op->xtype->code), (bool *)T.vals);
            });
        } else {
            int64_t zmask;
            const int o = op->opcode;
            const int64_t k = gb_iop_thunk_pos(o, y, ycode, op->ytype->code, &zmask);
            with_ztype(zcode, [&](auto zv) {
                using Z = decltype(zv);
                if (gb_iop_needs_row(o))
                    hipLaunchKernelGGL((k_apply_index<IDX_ROWCOL, int64_t, Z>), dim3(grid), dim3(IDX_BLOCK), 0,
                                       gb_stream(), v.nvals, v.nrows, o, v.rowptr, v.colidx,
                                       (const int64_t *)nullptr, k, (int64_t)0, (Z *)T.vals);
                else
                    hipLaunchKernelGGL((k_apply_index<IDX_COL, int64_t, Z>), dim3(grid), dim3(IDX_BLOCK), 0,
                                       gb_stream(), v.nvals, v.nrows, o, v.rowptr, v.colidx,
                                       (const int64_t *)nullptr, k, (int64_t)0, (Z *)T.vals);
            });
        }
        GB_LAUNCH_CHECK();
    }
    gb_writeback_matrix(C, T, M, d, accum);
}

}  // namespace

void gb_apply_index(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
                    const gb_desc &d) {
    GB_REQUIRE(op, GrB_NULL_POINTER, "operator is NULL");
    GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid operator");
    gb_check_binop(accum, true);
    GB_REQUIRE(op->opcode >= 0 && op->opcode < GBAMD_IOP_COUNT, GrB_INVALID_VALUE, "unknown index-unary operator");
    const int zcode = gb_iop_is_index(op->opcode) ? op->ytype->code : GBAMD_T_BOOL;
    if (C->kind != GB_KIND_MATRIX) apply_index_vector(C, M, accum, op, zcode, A, y, ycode, d);
    else apply_index_matrix(C, M, accum, op, zcode, A, y, ycode, d);
}

extern "C" {

#define GB_DEFINE_APPLY_INDEX(T, ctype)                                                                            \
    GrB_Info GrB_Matrix_apply_IndexOp_##T(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,           \
                                          const GrB_IndexUnaryOp op, const GrB_Matrix A, ctype y,                  \
                                          const GrB_Descriptor desc) {                                             \
        return gb_api(OBJ(C), [&] {                                                                                \
            gb_apply_index(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), &y, GBAMD_T_##T, \
                           gb_read_desc(desc));                                                                    \
        });                                                                                                        \
    }                                                                                                              \
    GrB_Info GrB_Vector_apply_IndexOp_##T(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,           \
                                          const GrB_IndexUnaryOp op, const GrB_Vector u, ctype y,                  \
                                          const GrB_Descriptor desc) {                                             \
        return gb_api(OBJ(w), [&] {                                                                                \
            gb_apply_index(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(u), &y, GBAMD_T_##T, \
                           gb_read_desc(desc));                                                                    \
        });                                                                                                        \
    }

GB_FOR_EACH_TYPE(GB_DEFINE_APPLY_INDEX)

}  // extern "C"
