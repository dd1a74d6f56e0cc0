// gb_subassign.hip -- writing an object into a region of a matrix or vector:
//   GxB_Matrix_subassign   C(I,J)<Mask,repl> = accum(C(I,J), A')   (reference core/matrix.py:3126-3316)
//   GxB_Vector_subassign   w(I)<mask,repl>   = accum(w(I), u)      (reference core/vector.py, "GxB_Vector_subassign")
//   GxB_Row_subassign / GxB_Col_subassign                          one row / column of C, mask of the region's size
//   GrB_Row_assign / GrB_Col_assign                                the same with a mask over the whole row / column
//   GxB_Matrix_subassign_Scalar / GxB_Vector_subassign_Scalar      a GrB_Scalar spread over the region
//
// Construction.  Inside the region the operation is an ordinary write-back on the submatrix
// S = C(I, J): the extract of gb_extract.hip, then gb_writeback_matrix on a temporary object.
// What is new here is putting S back:
//   placement       entry (r, c) of S keeps its row and gets column J[c]; when J does not ascend
//                   the rows are re-sorted by (r << 32 | J[c]) keys, as extract does;
//   region replace  row i of the result = C's entries of row i outside the region, merged with
//                   placed row rowsrc[i].  The two have disjoint ascending columns, so an entry's
//                   position is its rank in its own sequence plus a binary search in the other:
//                   entry-parallel, no atomics, no sort, the same bytes on every run.
// Vectors are bitmaps: s = w(I), the write-back on s, then one scatter of s's bits and values to
// the positions I (word-wide AND / OR atomics, whose result does not depend on their order).
// A row or column of C is handled as a vector and placed back as a 1 x n or n x 1 region.
// A repeated index in I or J is refused before anything is written.
#include <algorithm>
#include <vector>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SA_BLOCK 256
#define SA_GRID_CAP 16384
#define SA_WPI 4  // wave steps (64 entries each) to a chunk of the row search

// ------------------------------------------------------------------ kernels
// f(e, the row of e) for every entry e < nvals: a wave takes a run of chunks of SA_WPI * 64 entries and
// finds their rows with the shared wave row search (gb_chunk_rows), which skips runs of empty rows.
// The launch has SA_BLOCK threads to a block (sa_chunk_grid blocks)
template <class F>
__device__ __forceinline__ void sa_for_entries(const int64_t *__restrict__ rp, int64_t nrows, int64_t nvals, F &&f) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * SA_BLOCK) >> 6;
    const int64_t ngroups = (nvals + SA_WPI * 64 - 1) / (SA_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)SA_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;  // where the row search of the wave's previous chunk ended
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * (SA_WPI * 64);
        int64_t row[SA_WPI];
        gb_chunk_rows<SA_WPI>(rp, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < SA_WPI; u++) {
            const int64_t e = p0 + u * 64 + lane;
            if (e < nvals) f(e, row[u]);
        }
    }
}

// placement with an ascending J: the column of every entry of S in C
__global__ __launch_bounds__(SA_BLOCK) void k_sa_cols(int64_t snz, const int32_t *__restrict__ sci,
                                                      const int64_t *__restrict__ J, int32_t *__restrict__ pcol) {
    GB_GRID_LOOP(e, snz) pcol[e] = (int32_t)J[sci[e]];
}
// placement with any other J: sort keys (row of S << 32 | column in C) and the entry's position
__global__ __launch_bounds__(SA_BLOCK) void k_sa_keys(int64_t ni, int64_t snz, const int64_t *__restrict__ srp,
                                                      const int32_t *__restrict__ sci, const int64_t *__restrict__ J,
                                                      uint64_t *__restrict__ key, int64_t *__restrict__ src) {
    sa_for_entries(srp, ni, snz, [&](int64_t e, int64_t r) {
        key[e] = ((uint64_t)r << 32) | (uint64_t)(uint32_t)J[sci[e]];
        src[e] = e;
    });
}
template <class V>
__global__ __launch_bounds__(SA_BLOCK) void k_sa_unkey(int64_t snz, const uint64_t *__restrict__ key,
                                                       const int64_t *__restrict__ src, const V *__restrict__ vin,
                                                       int32_t *__restrict__ pcol, V *__restrict__ vout) {
    GB_GRID_LOOP(t, snz) {
        pcol[t] = (int32_t)(key[t] & 0xffffffffULL);
        if (vout) vout[t] = vin[src[t]];
    }
}

// rowsrc == nullptr: every row is in I (row i of S is row i of C); jbits == nullptr: every column is in J
__device__ __forceinline__ int64_t sa_src_row(const int32_t *__restrict__ rowsrc, int64_t i) {
    return rowsrc ? (int64_t)rowsrc[i] : i;
}

// flag[e] = entry e of C lies outside the region and is kept
__global__ __launch_bounds__(SA_BLOCK) void k_sa_flag(int64_t nrows, int64_t cnz, const int64_t *__restrict__ crp,
                                                      const int32_t *__restrict__ cci,
                                                      const int32_t *__restrict__ rowsrc,
                                                      const uint64_t *__restrict__ jbits, uint8_t *__restrict__ flag) {
    sa_for_entries(crp, nrows, cnz, [&](int64_t e, int64_t i) {
        const int32_t c = cci[e];
        const bool inside = sa_src_row(rowsrc, i) >= 0 && (!jbits || ((jbits[c >> 6] >> (c & 63)) & 1ULL));
        flag[e] = !inside;
    });
}

// cnt[i] = kept entries of C's row i + entries of the placed row
__global__ __launch_bounds__(SA_BLOCK) void k_sa_count(int64_t nrows, const int64_t *__restrict__ crp,
                                                       const int64_t *__restrict__ sc,
                                                       const int32_t *__restrict__ rowsrc,
                                                       const int64_t *__restrict__ prp, int64_t *__restrict__ cnt) {
    GB_GRID_LOOP(i, nrows) {
        const int64_t rs = sa_src_row(rowsrc, i);
        cnt[i] = sc[crp[i + 1]] - sc[crp[i]] + (rs >= 0 ? prp[rs + 1] - prp[rs] : 0);
    }
}

// a kept entry of C: its rank among the kept entries of its row + the placed columns below it
template <class V>
__global__ __launch_bounds__(SA_BLOCK) void k_sa_fill_c(int64_t nrows, int64_t cnz, const int64_t *__restrict__ crp,
                                                        const int32_t *__restrict__ cci, const V *__restrict__ cvx,
                                                        bool c_iso, const int64_t *__restrict__ sc,
                                                        const int32_t *__restrict__ rowsrc,
                                                        const int64_t *__restrict__ prp,
                                                        const int32_t *__restrict__ pcol,
                                                        const int64_t *__restrict__ orp, int32_t *__restrict__ oci,
                                                        V *__restrict__ ovx) {
    sa_for_entries(crp, nrows, cnz, [&](int64_t e, int64_t i) {
        if (sc[e + 1] == sc[e]) return;
        const int32_t c = cci[e];
        const int64_t rs = sa_src_row(rowsrc, i);
        int64_t below = 0;
        if (rs >= 0) {
            const int64_t a = prp[rs];
            below = gb_lower_bound(pcol, a, prp[rs + 1], c) - a;
        }
        const int64_t o = orp[i] + (sc[e] - sc[crp[i]]) + below;
        oci[o] = c;
        ovx[o] = cvx[c_iso ? 0 : e];
    });
}

// a placed entry: its rank in its row + the kept entries of C's row below its column
template <class V>
__global__ __launch_bounds__(SA_BLOCK) void k_sa_fill_p(int64_t ni, int64_t pnz, const int64_t *__restrict__ prp,
                                                        const int32_t *__restrict__ pcol, const V *__restrict__ pvx,
                                                        bool p_iso, const int64_t *__restrict__ I,
                                                        const int64_t *__restrict__ crp,
                                                        const int32_t *__restrict__ cci,
                                                        const int64_t *__restrict__ sc,
                                                        const int64_t *__restrict__ orp, int32_t *__restrict__ oci,
                                                        V *__restrict__ ovx) {
    sa_for_entries(prp, ni, pnz, [&](int64_t t, int64_t r) {
        const int64_t i = I ? I[r] : r;
        const int32_t c = pcol[t];
        const int64_t a = crp[i];
        const int64_t p = gb_lower_bound(cci, a, crp[i + 1], c);
        const int64_t o = orp[i] + (t - prp[r]) + (sc[p] - sc[a]);
        oci[o] = c;
        ovx[o] = pvx[p_iso ? 0 : t];
    });
}

// bit I[k] of w = bit k of s, and the value with it.  I holds no index twice, but several k
// share a word of w: AND / OR on the word, which commute
template <class V>
__global__ __launch_bounds__(SA_BLOCK) void k_sa_scatter(int64_t ni, const int64_t *__restrict__ I,
                                                         const uint64_t *__restrict__ sbits,
                                                         const V *__restrict__ svals, bool s_iso,
                                                         unsigned long long *__restrict__ wbits,
                                                         V *__restrict__ wvals) {
    GB_GRID_LOOP(k, ni) {
        const int64_t i = I[k];
        const unsigned long long bit = 1ULL << (i & 63);
        if ((sbits[k >> 6] >> (k & 63)) & 1ULL) {
            atomicOr(&wbits[i >> 6], bit);
            wvals[i] = svals[s_iso ? 0 : k];
        } else {
            atomicAnd(&wbits[i >> 6], ~bit);
        }
    }
}

// the structure of a full ni x nj matrix
__global__ __launch_bounds__(SA_BLOCK) void k_sa_full(int64_t ni, int64_t nj, int64_t *__restrict__ rp,
                                                      int32_t *__restrict__ ci) {
    GB_GRID_LOOP(r, ni + 1) rp[r] = r * nj;
    GB_GRID_LOOP(e, ni * nj) ci[e] = (int32_t)(e % nj);
}

// ------------------------------------------------------------------ host side
namespace {

// a temporary object, freed at scope exit
struct sa_tmp {
    GB_Obj *o = nullptr;
    explicit sa_tmp(GB_Obj *p) : o(p) {}
    sa_tmp(const sa_tmp &) = delete;
    ~sa_tmp() {
        if (o) {
            GrB_Matrix m = (GrB_Matrix)o;
            GrB_Matrix_free(&m);
        }
    }
};
// the buffers of a vector result the write-back did not take (it threw)
struct sa_vec_guard {
    gb_vec_result &T;
    ~sa_vec_guard() {
        gb_free(T.bits);
        gb_free(T.dense);
        gb_free(T.d_nvals);
    }
};
struct sa_mat_guard {
    gb_mat_result &T;
    ~sa_mat_guard() {
        gb_free(T.rowptr);
        gb_free(T.colidx);
        gb_free(T.vals);
    }
};

// blocks of a launch of sa_for_entries: a wave takes a run of chunks (4 or more, once there are that many)
unsigned sa_chunk_grid(int64_t nvals) {
    const int64_t ngroups = (nvals + SA_WPI * 64 - 1) / (SA_WPI * 64);
    return gb_grid((ngroups + 3) / 4, SA_BLOCK / 64, SA_GRID_CAP);
}

void sa_check_unique(const gb_index_list &L, int64_t n, const char *what) {
    if (L.all || L.n < 2) return;
    std::vector<uint8_t> seen(n, 0);
    for (int64_t i : L.idx) {
        GB_REQUIRE(!seen[i], GrB_INVALID_VALUE, std::string("repeated index in ") + what);
        seen[i] = 1;
    }
}

gb_index_list sa_all(int64_t n) {
    gb_index_list L;
    L.all = true;
    L.n = n;
    return L;
}
gb_index_list sa_one(int64_t i) {
    gb_index_list L;
    L.n = 1;
    L.idx.assign(1, i);
    return L;
}

int64_t *sa_upload(const gb_index_list &L, gb_scratch &s) {
    if (L.all || L.n == 0) return nullptr;
    int64_t *d = s.get<int64_t>(L.n);
    gb_copy_h2d(d, L.idx.data(), L.n * sizeof(int64_t));
    return d;
}

// C(I, J) = S, S of C's type with values svals (S.iso: one value): placement, then the region replace
void sa_place(GB_Obj *C, const gb_csr_view &S, const void *svals, const gb_index_list &LI, const gb_index_list &LJ) {
    gb_csr_view cv;
    gb_get_csr(cv, C);
    const int64_t nrows = cv.nrows, ncols = cv.ncols, cnz = cv.nvals, snz = S.nvals, ni = LI.n;
    GB_REQUIRE(ni < (1LL << 31) && LJ.n < (1LL << 31), GrB_NOT_IMPLEMENTED, "subassign of more than 2^31 rows/columns");
    GB_REQUIRE(S.nrows == ni && S.ncols == LJ.n, GrB_DIMENSION_MISMATCH, "region dimensions mismatch");
    const size_t ts = gb_type_size(C->type->code);
    gb_scratch s;
    // host tables, O(nrows + ncols): the inverse of I and the bitmap of J
    std::vector<int32_t> h_rowsrc;
    std::vector<uint64_t> h_jbits;
    const int64_t *dI = sa_upload(LI, s);
    const int64_t *dJ = sa_upload(LJ, s);
    const int32_t *rowsrc = nullptr;
    const uint64_t *jbits = nullptr;
    if (!LI.all) {
        h_rowsrc.assign(nrows, -1);
        for (int64_t k = 0; k < ni; k++) h_rowsrc[LI.idx[k]] = (int32_t)k;
        int32_t *d = s.get<int32_t>(nrows);
        gb_copy_h2d(d, h_rowsrc.data(), nrows * sizeof(int32_t));
        rowsrc = d;
    }
    bool j_sorted = true;
    if (!LJ.all) {
        h_jbits.assign(gb_words(ncols), 0);
        for (int64_t k = 0; k < LJ.n; k++) {
            h_jbits[LJ.idx[k] >> 6] |= 1ULL << (LJ.idx[k] & 63);
            if (k && LJ.idx[k] < LJ.idx[k - 1]) j_sorted = false;
        }
        uint64_t *d = s.get<uint64_t>(gb_words(ncols));
        gb_copy_h2d(d, h_jbits.data(), gb_words(ncols) * sizeof(uint64_t));
        jbits = d;
    }
    gb_stat_set("subassign_jsort", j_sorted ? 0 : 1);
    // ---- placement: pcol (and pvx when the rows were re-sorted)
    const int32_t *pcol = S.colidx;
    const void *pvx = svals;
    if (!LJ.all && snz) {
        int32_t *pc = s.get<int32_t>(snz);
        if (j_sorted) {
            hipLaunchKernelGGL(k_sa_cols, dim3(gb_grid(snz, SA_BLOCK, SA_GRID_CAP)), dim3(SA_BLOCK), 0, gb_stream(),
                               snz, S.colidx, dJ, pc);
            GB_LAUNCH_CHECK();
        } else {
            uint64_t *key = s.get<uint64_t>(snz);
            int64_t *src = s.get<int64_t>(snz);
            hipLaunchKernelGGL(k_sa_keys, dim3(sa_chunk_grid(snz)), dim3(SA_BLOCK), 0, gb_stream(),
                               ni, snz, S.rowptr, S.colidx, dJ, key, src);
            GB_LAUNCH_CHECK();
            int bits = 32;
            while (bits < 64 && (1LL << (bits - 32)) < ni) bits++;
            gb_sort_pairs_u64(key, src, snz, bits);
            void *pv = S.iso ? nullptr : s.get<char>(snz * ts);
            gb_with_size(ts, [&](auto z) {
                using V = decltype(z);
                hipLaunchKernelGGL((k_sa_unkey<V>), dim3(gb_grid(snz, SA_BLOCK, SA_GRID_CAP)), dim3(SA_BLOCK), 0,
                                   gb_stream(), snz, key, src, (const V *)svals, pc, (V *)pv);
            }, true);
            GB_LAUNCH_CHECK();
            if (pv) pvx = pv;
        }
        pcol = pc;
    }
    // ---- region replace: count, then fill
    uint8_t *flag = s.get<uint8_t>(std::max<int64_t>(cnz, 1));
    int64_t *sc = s.get<int64_t>(cnz + 1);
    if (cnz) {
        hipLaunchKernelGGL(k_sa_flag, dim3(sa_chunk_grid(cnz)), dim3(SA_BLOCK), 0, gb_stream(), nrows,
                           cnz, cv.rowptr, cv.colidx, rowsrc, jbits, flag);
        GB_LAUNCH_CHECK();
    }
    gb_exclusive_scan_u8(flag, sc, cnz);
    int64_t *cnt = s.get<int64_t>(nrows + 1);
    int64_t *orp = gb_malloc_n<int64_t>(nrows + 1);
    int32_t *oci = nullptr;
    void *ovx = nullptr;
    try {
        if (nrows) {
            hipLaunchKernelGGL(k_sa_count, dim3(gb_grid(nrows, SA_BLOCK, SA_GRID_CAP)), dim3(SA_BLOCK), 0, gb_stream(),
                               nrows, cv.rowptr, sc, rowsrc, S.rowptr, cnt);
            GB_LAUNCH_CHECK();
        }
        gb_exclusive_scan_i64(cnt, orp, nrows);
        const int64_t nz = gb_read_i64(orp + nrows);  // also: the host tables above have been read
        oci = gb_malloc_n<int32_t>(std::max<int64_t>(nz, 1));
        ovx = gb_malloc(std::max<int64_t>(nz, 1) * ts);
        gb_with_size(ts, [&](auto z) {
            using V = decltype(z);
            if (cnz)
                hipLaunchKernelGGL((k_sa_fill_c<V>), dim3(sa_chunk_grid(cnz)), dim3(SA_BLOCK), 0,
                                   gb_stream(), nrows, cnz, cv.rowptr, cv.colidx, (const V *)cv.vals, cv.iso, sc, rowsrc,
                                   S.rowptr, pcol, orp, oci, (V *)ovx);
            if (snz)
                hipLaunchKernelGGL((k_sa_fill_p<V>), dim3(sa_chunk_grid(snz)), dim3(SA_BLOCK), 0,
                                   gb_stream(), ni, snz, S.rowptr, pcol, (const V *)pvx, S.iso, dI, cv.rowptr, cv.colidx,
                                   sc, orp, oci, (V *)ovx);
        }, true);
        GB_LAUNCH_CHECK();
        gb_install_csr(C, nrows, ncols, nz, orp, oci, ovx, false);
    } catch (...) {
        gb_free(orp);
        gb_free(oci);
        gb_free(ovx);
        throw;
    }
}

gb_vec_result sa_copy_bitmap(const gb_bitmap_view &v) {
    gb_vec_result T = gb_new_vec_result(v.n, v.tcode, v.iso);
    const size_t ts = gb_type_size(v.tcode);
    if (v.n) {
        gb_copy_d2d(T.bits, v.bits, gb_words(v.n) * sizeof(uint64_t));
        gb_copy_d2d(T.dense, v.vals, (v.iso ? 1 : v.n) * ts);
    }
    gb_bitmap_count(T.bits, v.n, T.d_nvals);
    return T;
}

// w(I)<mask, replace> = accum(w(I), U); U has LI.n positions and is consumed
void sa_vector(GB_Obj *W, GB_Obj *M, GrB_BinaryOp accum, gb_vec_result &U, const gb_index_list &LI,
               const gb_desc &d) {
    sa_vec_guard guard{U};
    const int64_t n = W->nrows, ni = LI.n;
    GB_REQUIRE(U.n == ni, GrB_DIMENSION_MISMATCH, "u size does not match the index list");
    GB_REQUIRE(!M || (M->nrows == ni && gb_ncols_of(M) == 1), GrB_DIMENSION_MISMATCH,
               "mask size does not match the index list");
    if (LI.all) {  // the region is all of w
        gb_writeback_vector(W, U, M, d, accum, false);
        return;
    }
    sa_tmp S(gb_new_object(GB_KIND_VECTOR, W->type, ni, 1));
    {
        gb_bitmap_view wv;
        gb_get_bitmap(wv, W);
        gb_vec_result T;
        gb_extract_vec(T, wv, LI);
        gb_install_bitmap(S.o, ni, T.bits, T.dense, T.iso, T.d_nvals);
    }
    gb_writeback_vector(S.o, U, M, d, accum, false);
    if (ni == 0) return;
    // a copy of w with s scattered into it (w may be the mask or u: they have been read)
    gb_bitmap_view wv, sv;
    gb_get_bitmap(wv, W);
    gb_get_bitmap(sv, S.o);
    const size_t ts = W->type->size;
    gb_scratch s;
    const int64_t *dI = sa_upload(LI, s);
    uint64_t *obits = gb_malloc_n<uint64_t>(gb_words(n));
    void *ovals = nullptr;
    try {
        gb_copy_d2d(obits, wv.bits, gb_words(n) * sizeof(uint64_t));
        if (wv.iso) {
            ovals = gb_expand_iso(wv.vals, ts, n);
        } else {
            ovals = gb_malloc(n * ts);
            gb_copy_d2d(ovals, wv.vals, n * ts);
        }
        gb_with_size(ts, [&](auto z) {
            using V = decltype(z);
            hipLaunchKernelGGL((k_sa_scatter<V>), dim3(gb_grid(ni, SA_BLOCK, SA_GRID_CAP)), dim3(SA_BLOCK), 0,
                               gb_stream(), ni, dI, sv.bits, (const V *)sv.vals, sv.iso, (unsigned long long *)obits,
                               (V *)ovals);
        }, true);
        GB_LAUNCH_CHECK();
        gb_sync();  // the index list on the host has been read
        gb_install_bitmap(W, n, obits, ovals, false, nullptr);
    } catch (...) {
        gb_free(obits);
        gb_free(ovals);
        throw;
    }
}

// one row (col == false) or column of C as a vector of C's type
void sa_take_line(GB_Obj *Z, GB_Obj *C, bool col, int64_t idx) {
    gb_csr_view cv;
    gb_get_csr(cv, C);
    if (col) {  // C(:, idx) as an n x 1 CSR, which the install turns into a bitmap
        gb_mat_result T;
        gb_extract_csr(T, cv, sa_all(cv.nrows), sa_one(idx));
        gb_install_csr(Z, cv.nrows, 1, T.nvals, T.rowptr, T.colidx, T.vals, T.iso);
    } else {
        gb_vec_result T;
        gb_extract_line(T, cv, idx, sa_all(cv.ncols));
        gb_install_bitmap(Z, cv.ncols, T.bits, T.dense, T.iso, T.d_nvals);
    }
}

// the row / column forms.  subassign: z = the line; z(L)<mask, repl> = accum(z(L), u); the line = z.
// assign: z(L) = accum(z(L), u) without a mask, then line<mask, repl> = z with the mask over the whole line
void sa_line(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GB_Obj *U, bool col, GrB_Index idx, const GrB_Index *L,
             GrB_Index nl, const gb_desc &d, bool assign) {
    gb_check_binop(accum, true);
    const int64_t nrows = C->nrows, ncols = gb_ncols_of(C);
    const int64_t len = col ? nrows : ncols;
    GB_REQUIRE(idx < (GrB_Index)(col ? ncols : nrows), GrB_INVALID_INDEX,
               col ? "column index out of bounds" : "row index out of bounds");
    gb_index_list LL;
    gb_expand_indices(LL, L, nl, len);
    sa_check_unique(LL, len, col ? "I" : "J");
    GB_REQUIRE(U->nrows == LL.n && gb_ncols_of(U) == 1, GrB_DIMENSION_MISMATCH, "u size does not match the index list");
    GB_REQUIRE(!M || (M->nrows == (assign ? len : LL.n) && gb_ncols_of(M) == 1), GrB_DIMENSION_MISMATCH,
               assign ? "mask size does not match the row / column of C" : "mask size does not match the index list");
    gb_stat_set("subassign_extract", 1);
    sa_tmp Z(gb_new_object(GB_KIND_VECTOR, C->type, len, 1));
    sa_take_line(Z.o, C, col, (int64_t)idx);
    gb_vec_result Uc;
    {
        gb_bitmap_view uv;
        gb_get_bitmap(uv, U);
        Uc = sa_copy_bitmap(uv);
    }
    GB_Obj *res = Z.o;
    sa_tmp R(nullptr);
    if (!assign) {
        sa_vector(Z.o, M, accum, Uc, LL, d);
    } else {
        sa_vector(Z.o, nullptr, accum, Uc, LL, gb_desc{});
        if (M || d.comp) {
            R.o = gb_new_object(GB_KIND_VECTOR, C->type, len, 1);
            sa_take_line(R.o, C, col, (int64_t)idx);
            gb_bitmap_view zv;
            gb_get_bitmap(zv, Z.o);
            gb_vec_result T = sa_copy_bitmap(zv);
            sa_vec_guard guard{T};
            gb_writeback_vector(R.o, T, M, d, nullptr, false);
            res = R.o;
        }
    }
    gb_csr_view sv;
    if (col) {
        gb_get_csr(sv, res);  // len x 1
        sa_place(C, sv, sv.vals, sa_all(nrows), sa_one((int64_t)idx));
    } else {
        gb_get_csc(sv, res);  // 1 x len
        sa_place(C, sv, sv.vals, sa_one((int64_t)idx), sa_all(ncols));
    }
}

// C(I, J)<Mask, replace> = accum(C(I, J), A) for a view A of the region's shape
void sa_matrix(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, gb_csr_view &av, const gb_index_list &LI,
               const gb_index_list &LJ, const gb_desc &d) {
    const int64_t ni = LI.n, nj = LJ.n;
    GB_REQUIRE(av.nrows == ni && av.ncols == nj, GrB_DIMENSION_MISMATCH, "A does not have the region's shape");
    GB_REQUIRE(!M || (M->nrows == ni && gb_ncols_of(M) == nj), GrB_DIMENSION_MISMATCH,
               "mask does not have the region's shape");
    const int ct = C->type->code;
    if (!M && !d.comp && !accum) {  // S = A cast to C's type: no extract, no merge
        gb_stat_set("subassign_extract", 0);
        gb_scratch s;
        const void *vals = gb_view_vals_as(av, ct, s);
        sa_place(C, av, vals, LI, LJ);
        return;
    }
    gb_stat_set("subassign_extract", 1);
    sa_tmp S(gb_new_object(GB_KIND_MATRIX, C->type, ni, nj));
    {
        gb_csr_view cv;
        gb_get_csr(cv, C);
        gb_mat_result T;
        gb_extract_csr(T, cv, LI, LJ);
        gb_install_csr(S.o, ni, nj, T.nvals, T.rowptr, T.colidx, T.vals, T.iso);
    }
    {
        gb_mat_result T = gb_new_mat_result(ni, nj, av.tcode, av.nvals, av.iso);
        sa_mat_guard guard{T};
        gb_copy_d2d(T.rowptr, av.rowptr, (ni + 1) * sizeof(int64_t));
        if (av.nvals) {
            gb_copy_d2d(T.colidx, av.colidx, av.nvals * sizeof(int32_t));
            gb_copy_d2d(T.vals, av.vals, (av.iso ? 1 : av.nvals) * gb_type_size(av.tcode));
        }
        gb_writeback_matrix(S.o, T, M, d, accum);
    }
    gb_csr_view sv;
    gb_get_csr(sv, S.o);
    sa_place(C, sv, sv.vals, LI, LJ);
}

// the lists of a matrix form, checked
void sa_lists(gb_index_list &LI, gb_index_list &LJ, GB_Obj *C, const GrB_Index *I, GrB_Index ni, const GrB_Index *J,
              GrB_Index nj) {
    gb_expand_indices(LI, I, ni, C->nrows);
    gb_expand_indices(LJ, J, nj, gb_ncols_of(C));
    sa_check_unique(LI, C->nrows, "I");
    sa_check_unique(LJ, gb_ncols_of(C), "J");
}

}  // namespace

extern "C" {

GrB_Info GxB_Matrix_subassign(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A,
                              const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj,
                              const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *Ao = gb_obj_check(A), *Mo = gb_obj_check(Mask, true);
        gb_check_binop(accum, true);
        const gb_desc d = gb_read_desc(desc);
        gb_index_list LI, LJ;
        sa_lists(LI, LJ, Co, I, ni, J, nj);
        gb_csr_view av;
        if (d.tran0) gb_get_csc(av, Ao);
        else gb_get_csr(av, Ao);
        sa_matrix(Co, Mo, accum, av, LI, LJ, d);
    });
}

GrB_Info GxB_Matrix_subassign_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                     const GrB_Scalar x, const GrB_Index *I, GrB_Index ni, const GrB_Index *J,
                                     GrB_Index nj, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *Xo = gb_obj_check(x), *Mo = gb_obj_check(Mask, true);
        gb_check_binop(accum, true);
        const gb_desc d = gb_read_desc(desc);
        gb_index_list LI, LJ;
        sa_lists(LI, LJ, Co, I, ni, J, nj);
        // A = the scalar at every position of the region (iso), or no entry when it is empty
        gb_bitmap_view xv;
        gb_get_bitmap(xv, Xo);
        const bool present = gb_nvals(Xo) > 0;
        const int64_t nz = present ? LI.n * LJ.n : 0;
        gb_csr_view av;
        av.nrows = LI.n;
        av.ncols = LJ.n;
        av.nvals = nz;
        av.tcode = xv.tcode;
        av.iso = nz > 0;
        int64_t *rp = av.own.get<int64_t>(LI.n + 1);
        int32_t *ci = av.own.get<int32_t>(nz);
        void *vx = av.own.get<char>(gb_type_size(xv.tcode));
        if (nz) {
            hipLaunchKernelGGL(k_sa_full, dim3(gb_grid(nz, SA_BLOCK, SA_GRID_CAP)), dim3(SA_BLOCK), 0, gb_stream(), LI.n,
                               LJ.n, rp, ci);
            GB_LAUNCH_CHECK();
            gb_copy_d2d(vx, xv.vals, gb_type_size(xv.tcode));
        } else {
            gb_memset(rp, 0, (LI.n + 1) * sizeof(int64_t));
        }
        av.rowptr = rp;
        av.colidx = ci;
        av.vals = vx;
        sa_matrix(Co, Mo, accum, av, LI, LJ, d);
    });
}

GrB_Info GxB_Vector_subassign(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                              const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_Obj *W = gb_obj_check(w), *U = gb_obj_check(u), *Mo = gb_obj_check(mask, true);
        gb_check_binop(accum, true);
        const gb_desc d = gb_read_desc(desc);
        GB_REQUIRE(gb_ncols_of(W) == 1, GrB_DIMENSION_MISMATCH, "not a vector");
        gb_index_list LI;
        gb_expand_indices(LI, I, ni, W->nrows);
        sa_check_unique(LI, W->nrows, "I");
        GB_REQUIRE(U->nrows == LI.n && gb_ncols_of(U) == 1, GrB_DIMENSION_MISMATCH,
                   "u size does not match the index list");
        gb_bitmap_view uv;
        gb_get_bitmap(uv, U);
        gb_vec_result T = sa_copy_bitmap(uv);
        sa_vector(W, Mo, accum, T, LI, d);
    });
}

GrB_Info GxB_Vector_subassign_Scalar(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                                     const GrB_Scalar x, const GrB_Index *I, GrB_Index ni,
                                     const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_Obj *W = gb_obj_check(w), *Xo = gb_obj_check(x), *Mo = gb_obj_check(mask, true);
        gb_check_binop(accum, true);
        const gb_desc d = gb_read_desc(desc);
        GB_REQUIRE(gb_ncols_of(W) == 1, GrB_DIMENSION_MISMATCH, "not a vector");
        gb_index_list LI;
        gb_expand_indices(LI, I, ni, W->nrows);
        sa_check_unique(LI, W->nrows, "I");
        gb_bitmap_view xv;
        gb_get_bitmap(xv, Xo);
        const bool present = gb_nvals(Xo) > 0;
        // u = the scalar at every position of the list (iso), or no entry when it is empty
        gb_vec_result T = gb_new_vec_result(LI.n, xv.tcode, true);
        const int64_t nw = gb_words(LI.n);
        std::vector<uint64_t> hb(nw, present ? ~0ULL : 0ULL);
        if (present && (LI.n & 63)) hb[nw - 1] = (1ULL << (LI.n & 63)) - 1;
        const int64_t cnt = present ? LI.n : 0;
        gb_copy_h2d(T.bits, hb.data(), nw * sizeof(uint64_t));
        gb_copy_h2d(T.d_nvals, &cnt, sizeof(int64_t));
        gb_copy_d2d(T.dense, xv.vals, gb_type_size(xv.tcode));
        gb_sync();
        sa_vector(W, Mo, accum, T, LI, d);
    });
}

GrB_Info GxB_Row_subassign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                           GrB_Index i, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *U = gb_obj_check(u), *Mo = gb_obj_check(mask, true);
        sa_line(Co, Mo, accum, U, false, i, J, nj, gb_read_desc(desc), false);
    });
}
GrB_Info GxB_Col_subassign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                           const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *U = gb_obj_check(u), *Mo = gb_obj_check(mask, true);
        sa_line(Co, Mo, accum, U, true, j, I, ni, gb_read_desc(desc), false);
    });
}
GrB_Info GrB_Row_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                        GrB_Index i, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *U = gb_obj_check(u), *Mo = gb_obj_check(mask, true);
        sa_line(Co, Mo, accum, U, false, i, J, nj, gb_read_desc(desc), true);
    });
}
GrB_Info GrB_Col_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                        const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *U = gb_obj_check(u), *Mo = gb_obj_check(mask, true);
        sa_line(Co, Mo, accum, U, true, j, I, ni, gb_read_desc(desc), true);
    });
}

}  // extern "C"
