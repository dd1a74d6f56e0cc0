// gb_reindex.hip -- the operations that keep every stored value and change the index it sits at:
//   GrB_Matrix_diag / GxB_Matrix_diag    reference core/vector.py:620-642, core/ss/matrix.py:252-279
//   GxB_Vector_diag                      reference core/matrix.py:735-754, core/ss/vector.py:147-183
//   GxB_Matrix_reshape / _reshapeDup     reference core/ss/matrix.py:3742-3815, core/ss/vector.py:1377-1405
//   GxB_Vector_flatten                   reference core/ss/matrix.py:3717-3740 (this backend's own entry point:
//                                        a vector is a bitmap here, no n x 1 matrix cast gives one)
//   GxB_{Matrix,Vector}_import_dense     reference core/matrix.py:1457-1518, core/vector.py:894-946
//   GxB_{Matrix,Vector}_export_dense     reference core/matrix.py:1520-1574, core/vector.py:948-999
//                                        (this backend's own names: a dense array, host or device,
//                                        in and out; the layout is stated with the code below)
// No mask, no accumulator; the output's old contents are discarded.
//
// Layout formulas.  A vector is a bitmap with dense values; rank(p) = the entries below position p
// = woff[p >> 6] + popcount(bits[p >> 6] & the bits below p & 63), woff the exclusive scan of the
// words' popcounts (rank(size) = nvals).
//   diagonal matrix   v(p) sits at (p + r0, p + c0), r0 = max(-k, 0), c0 = max(k, 0), in storage
//                     position rank(p); row r holds position r - r0 alone, so rowptr[r] =
//                     rank(clamp(r - r0, 0, size)): 0 above the vector's span, nvals below it
//   vector reshape    row-major into nr x nc: v(p) sits at (p / nc, p % nc), storage position
//                     rank(p); rowptr[r] = rank(r * nc)
//   diagonal vector   w(p) = A(p + r0, p + c0): one search of column p + c0 in row p + r0
//   matrix reshape    row-major, (i, j) -> divmod(lin, nc'), lin = i * nc + j.  lin grows along the
//                     CSR's storage order, so every entry keeps its storage position: the values do
//                     not move, colidx'[p] = lin % nc', and rowptr'[r'] = the first entry with
//                     lin >= r' * nc' = rowptr[i0] + lower_bound(columns of row i0, j0) with
//                     (i0, j0) = divmod(r' * nc', nc)
//   flatten           w(lin) = A(i, j), lin = i * nc + j (row-major) or i + j * nr (column-major)
// A column-major reshape (lin = i + j * nr, entry at (lin % nr', lin / nr')) is the row-major
// reshape of the transpose into nc' x nr', transposed back: it runs the same kernels on
// gb_get_csc's view (a bitmap is its own column-major order) and ends in gb_transpose_csr.
//
// Kernels (wave64, no scan beyond the words' popcounts, no row-of-entry array):
//   k_bitmap_csr      one lane per bitmap position: a set bit writes its column and value at its
//                     rank; then one lane per row writes the row pointer.  No atomics
//   k_csr_diag        one lane per diagonal position, one binary search each (a hub row costs one
//                     search, it is not walked); the wave's ballot is the output bitmap word, so
//                     the last word has no bit at or past the size
//   k_reshape_cols    one lane per entry, the old row from gb_chunk_rows, one division by the
//                     launch's one divisor: 32-bit when nrows * ncols < 2^32, else 64-bit
//                     ("stat_reshape_div64" = 1 when the last reshape took the 64-bit path)
//   k_reshape_rowptr  one lane per new row, the closed form above
//   k_flatten         one lane per entry into a zeroed bitmap: atomicOr on the entry's word, the
//                     value stored at lin.  The atomic has no reader (no return value is used),
//                     serves both orders with one kernel (column-major entries of one word are not
//                     neighbours in storage) and words shared by two waves need it in any case
//   k_dense_flags     one lane per position of a dense array, the wave's ballot of "holds an
//                     entry" is the bitmap word that k_bitmap_csr then reads
//   k_dense_fill      the fill value over a whole array in 16-byte stores
//   k_dense_scatter   one lane per entry, the row from gb_chunk_rows, the value stored at
//                     row * ncols + col.  Positions are unique: no atomics
//   k_bitmap_dense    one lane per position of a vector: its value or the fill, and its bit as a byte
#include <algorithm>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define RIX_BLOCK 256
#define RIX_WPI 4  // wave steps (64 entries each) to a chunk
#define RIX_GRID_CAP 8192

namespace {

typedef unsigned __int128 u128;

GB_DEV int64_t rix_rank(const uint64_t *__restrict__ bits, const int64_t *__restrict__ woff, int64_t p) {
    return woff[p >> 6] + __popcll(bits[p >> 6] & ((1ULL << (p & 63)) - 1));
}

__global__ __launch_bounds__(RIX_BLOCK) void k_word_popcount(const uint64_t *__restrict__ bits, int64_t nw,
                                                             int64_t *__restrict__ pop) {
    GB_GRID_LOOP(w, nw) pop[w] = __popcll(bits[w]);
}

// Bitmap of n positions (nw words, woff[nw] = nvals) to the CSR of nrows rows under a position
// map.  DIAG: position p -> (p + r0, p + c); else p -> (p / c, p % c), IX the width of the
// division.  vx == nullptr: the values are not moved (iso).
template <bool DIAG, class IX, class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_bitmap_csr(int64_t n, int64_t nw, const uint64_t *__restrict__ bits,
                                                          const W *__restrict__ dense,
                                                          const int64_t *__restrict__ woff, int64_t nrows, int64_t r0,
                                                          int64_t c, int64_t *__restrict__ rp,
                                                          int32_t *__restrict__ ci, W *__restrict__ vx) {
    GB_GRID_LOOP(p, n) {
        const uint64_t word = bits[p >> 6];
        const int b = (int)(p & 63);
        if (!((word >> b) & 1ULL)) continue;
        const int64_t rank = woff[p >> 6] + __popcll(word & ((1ULL << b) - 1));
        ci[rank] = DIAG ? (int32_t)(p + c) : (int32_t)((IX)p % (IX)c);
        if (vx) vx[rank] = dense[p];
    }
    GB_GRID_LOOP(r, nrows + 1) {
        int64_t p = DIAG ? r - r0 : r * c;  // the row's first position (r * c <= n)
        p = p < 0 ? 0 : p;
        rp[r] = p >= n ? woff[nw] : rix_rank(bits, woff, p);
    }
}

// w(p) = A(p + r0, p + c0) for p in [0, size); vx == nullptr: the values are not moved (iso)
template <class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_csr_diag(int64_t size, int64_t r0, int64_t c0,
                                                        const int64_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ ci, const W *__restrict__ vx,
                                                        uint64_t *__restrict__ obits, W *__restrict__ dense) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (size + 63) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * RIX_BLOCK) >> 6;
    for (int64_t w = (blockIdx.x * (int64_t)RIX_BLOCK + threadIdx.x) >> 6; w < nw; w += nwaves) {
        const int64_t p = (w << 6) + lane;
        bool hit = false;
        int64_t pos = 0;
        if (p < size) {
            const int64_t hi = rowptr[p + r0 + 1];
            const int64_t j = p + c0;
            pos = gb_lower_bound(ci, rowptr[p + r0], hi, j);
            hit = pos < hi && ci[pos] == j;
        }
        const unsigned long long word = __ballot(hit);
        if (lane == 0) obits[w] = word;
        if (hit && vx) dense[p] = vx[pos];
    }
}

// oci[p] = (row(p) * ncols + ci[p]) % ncols_new
template <class IX>
__global__ __launch_bounds__(RIX_BLOCK) void k_reshape_cols(int64_t nvals, int64_t nrows, IX ncols, IX ncols_new,
                                                            const int64_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ ci,
                                                            int32_t *__restrict__ oci) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * RIX_BLOCK) >> 6;
    const int64_t ngroups = (nvals + RIX_WPI * 64 - 1) / (RIX_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)RIX_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;  // where the row search of the wave's previous chunk ended
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * (RIX_WPI * 64);
        int64_t row[RIX_WPI];
        gb_chunk_rows<RIX_WPI>(rowptr, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= nvals) continue;
            const IX lin = (IX)row[u] * ncols + (IX)ci[p];
            oci[p] = (int32_t)(lin % ncols_new);
        }
    }
}

// orp[r] = the first entry at or after linear position r * ncols_new (ncols_new >= 1)
template <class IX>
__global__ __launch_bounds__(RIX_BLOCK) void k_reshape_rowptr(int64_t nrows_new, int64_t nvals, IX ncols,
                                                              IX ncols_new, const int64_t *__restrict__ rowptr,
                                                              const int32_t *__restrict__ ci,
                                                              int64_t *__restrict__ orp) {
    GB_GRID_LOOP(r, nrows_new + 1) {
        if (r == nrows_new) {
            orp[r] = nvals;
            continue;
        }
        const IX lin0 = (IX)r * ncols_new;
        const IX i0 = lin0 / ncols;
        const int32_t j0 = (int32_t)(lin0 - i0 * ncols);
        orp[r] = gb_lower_bound(ci, rowptr[i0], rowptr[i0 + 1], j0);
    }
}

// entry (i, j) goes to position i * mi + j * mj; vx == nullptr: the values are not moved (iso)
template <class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_flatten(int64_t nvals, int64_t nrows, int64_t mi, int64_t mj,
                                                       const int64_t *__restrict__ rowptr,
                                                       const int32_t *__restrict__ ci, const W *__restrict__ vx,
                                                       unsigned long long *__restrict__ bits, W *__restrict__ dense) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * RIX_BLOCK) >> 6;
    const int64_t ngroups = (nvals + RIX_WPI * 64 - 1) / (RIX_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)RIX_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, ngroups);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * (RIX_WPI * 64);
        int64_t row[RIX_WPI];
        gb_chunk_rows<RIX_WPI>(rowptr, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= nvals) continue;
            const int64_t lin = row[u] * mi + (int64_t)ci[p] * mj;
            atomicOr(&bits[lin >> 6], 1ULL << (lin & 63));
            if (vx) dense[lin] = vx[p];
        }
    }
}

// ------------------------------------------------------------------ dense import / export
// the run of chunks [g0, g1) of RIX_WPI * 64 items that this thread's wave takes out of n items
GB_DEV void rix_wave_chunks(int64_t n, int64_t &g0, int64_t &g1) {
    const int64_t nwaves = ((int64_t)gridDim.x * RIX_BLOCK) >> 6;
    const int64_t ngroups = (n + RIX_WPI * 64 - 1) / (RIX_WPI * 64);
    const int64_t per_wave = (ngroups + nwaves - 1) / nwaves;
    g0 = ((blockIdx.x * (int64_t)RIX_BLOCK + threadIdx.x) >> 6) * per_wave;
    g1 = min(g0 + per_wave, ngroups);
}

// bits[p >> 6] bit p & 63 = position p of the dense array holds an entry: its byte of Ab (when
// given) is not 0 and its value is != m (when has_m).  C: the type `!=` is C's in -- float and
// double for the float types (NaN != NaN, -0 == 0), the unsigned word for the others.  A wave
// per 64 positions, its ballot the word: no bit at or past n
template <class C>
__global__ __launch_bounds__(RIX_BLOCK) void k_dense_flags(int64_t n, const C *__restrict__ X,
                                                           const int8_t *__restrict__ Ab, bool has_m, C m,
                                                           uint64_t *__restrict__ bits) {
    const int lane = threadIdx.x & 63;
    int64_t g0, g1;
    rix_wave_chunks(n, g0, g1);
    for (int64_t g = g0; g < g1; g++) {
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t w0 = g * (RIX_WPI * 64) + u * 64, p = w0 + lane;
            if (w0 >= n) break;  // the wave as one
            bool keep = p < n;
            if (keep && Ab) keep = Ab[p] != 0;
            if (keep && has_m) keep = X[p] != m;
            const unsigned long long word = __ballot(keep);
            if (lane == 0) bits[w0 >> 6] = word;
        }
    }
}

// x[0 .. n) = val: 16-byte stores between the first and the last 16-byte boundary, the (fewer
// than 16 / sizeof(W)) elements before and after them by the first wave's lanes
template <class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_dense_fill(int64_t n, W *__restrict__ x, W val) {
    constexpr int64_t PER = 16 / sizeof(W);
    const int lane = threadIdx.x & 63;
    const int64_t head = min(n, (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(W)));
    const int64_t nvec = (n - head) / PER, tail0 = head + nvec * PER;
    uint64_t rep = (uint64_t)val;
#pragma unroll
    for (int s = 8 * sizeof(W); s < 64; s *= 2) rep |= rep << s;
    const ulonglong2 pat = make_ulonglong2(rep, rep);
    ulonglong2 *__restrict__ xv = (ulonglong2 *)(x + head);
    int64_t g0, g1;
    rix_wave_chunks(nvec, g0, g1);
    for (int64_t g = g0; g < g1; g++) {
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t i = g * (RIX_WPI * 64) + u * 64 + lane;
            if (i < nvec) xv[i] = pat;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        if (lane < head) x[lane] = val;
        if (tail0 + lane < n) x[tail0 + lane] = val;
    }
}

// entry (i, j) -> X[i * ncols + j] (and 1 into its byte of Ab, when given); iso: vx holds one value
template <class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_dense_scatter(int64_t nvals, int64_t nrows, int64_t ncols,
                                                             const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ ci, const W *__restrict__ vx,
                                                             bool iso, W *__restrict__ X, int8_t *__restrict__ Ab) {
    const int lane = threadIdx.x & 63;
    int64_t g0, g1;
    rix_wave_chunks(nvals, g0, g1);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * (RIX_WPI * 64);
        int64_t row[RIX_WPI];
        gb_chunk_rows<RIX_WPI>(rowptr, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= nvals) continue;
            const int64_t lin = row[u] * ncols + (int64_t)ci[p];
            X[lin] = vx[iso ? 0 : p];
            if (Ab) Ab[lin] = 1;
        }
    }
}

// a vector's bitmap to a dense array: X[p] = bit p ? dense[p] (dense[0] when iso) : fill, Ab[p] = bit p
template <class W>
__global__ __launch_bounds__(RIX_BLOCK) void k_bitmap_dense(int64_t n, const uint64_t *__restrict__ bits,
                                                            const W *__restrict__ dense, bool iso, W fill,
                                                            W *__restrict__ X, int8_t *__restrict__ Ab) {
    const int lane = threadIdx.x & 63;
    int64_t g0, g1;
    rix_wave_chunks(n, g0, g1);
    for (int64_t g = g0; g < g1; g++) {
#pragma unroll
        for (int u = 0; u < RIX_WPI; u++) {
            const int64_t p = g * (RIX_WPI * 64) + u * 64 + lane;
            if (p >= n) continue;
            const bool bit = (bits[p >> 6] >> lane) & 1ULL;
            X[p] = bit ? dense[iso ? 0 : p] : fill;
            if (Ab) Ab[p] = bit;
        }
    }
}

// ------------------------------------------------------------------ host side
// a wave takes a run of chunks (4 or more, once there are that many)
unsigned chunk_grid(int64_t nvals) {
    const int64_t ngroups = (nvals + RIX_WPI * 64 - 1) / (RIX_WPI * 64);
    return gb_grid((ngroups + 3) / 4, RIX_BLOCK / 64, RIX_GRID_CAP);
}

// an object made by gb_new_object_bare that nobody was handed
void free_bare(GB_Obj *o) {
    gb_obj_free_storage(o);
    gb_free(o->d_nvals);
    gb_host_slot_release(o->pub);
    o->magic = GB_FREED;
    delete o;
}

// T.vals as type `code`
void cast_result(gb_mat_result &T, int code) {
    if (T.tcode == code) return;
    const int64_t n = T.iso ? 1 : T.nvals;
    void *vx = gb_malloc((n < 1 ? 1 : n) * gb_type_size(code));
    gb_cast_array(vx, code, T.vals, T.tcode, n);
    gb_free(T.vals);
    T.vals = vx;
    T.tcode = code;
}

// The CSR of nrows x ncols that holds the bitmap u under a position map (values in u's type).
// diag: p -> (p + r0, p + c); else p -> (p / c, p % c) with nrows * c == u.n
gb_mat_result bitmap_csr(gb_bitmap_view &u, bool diag, int64_t nrows, int64_t ncols, int64_t r0, int64_t c) {
    const int64_t n = u.n, nw = gb_words(n);
    if (n == 0) return gb_empty_mat_result(nrows, ncols, u.tcode);
    gb_scratch s;
    int64_t *pop = s.get<int64_t>(nw), *woff = s.get<int64_t>(nw + 1);
    hipLaunchKernelGGL(k_word_popcount, dim3(gb_grid(nw, RIX_BLOCK, RIX_GRID_CAP)), dim3(RIX_BLOCK), 0, gb_stream(),
                       u.bits, nw, pop);
    GB_LAUNCH_CHECK();
    gb_exclusive_scan_i64(pop, woff, nw);
    const int64_t nz = u.h_nvals >= 0 ? u.h_nvals : gb_read_i64(woff + nw);
    const bool iso = u.iso && nz > 0;
    gb_mat_result T = gb_new_mat_result(nrows, ncols, u.tcode, nz, iso);
    if (iso) gb_copy_d2d(T.vals, u.vals, gb_type_size(u.tcode));
    const bool wide = !diag && n > (int64_t)UINT32_MAX;
    const unsigned grid = gb_grid(std::max(n, nrows + 1), RIX_BLOCK, RIX_GRID_CAP);
    gb_with_size(gb_type_size(u.tcode), [&](auto w) {
        using W = decltype(w);
        const W *dense = (const W *)u.vals;
        W *vx = iso || nz == 0 ? nullptr : (W *)T.vals;
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(RIX_BLOCK), 0, gb_stream(), n, nw, u.bits, dense,
                               (const int64_t *)woff, nrows, r0, c, T.rowptr, T.colidx, vx);
        };
        if (diag) go(k_bitmap_csr<true, uint32_t, W>);
        else if (wide) go(k_bitmap_csr<false, uint64_t, W>);
        else go(k_bitmap_csr<false, uint32_t, W>);
    });
    GB_LAUNCH_CHECK();
    return T;
}

// r0, c0 of diagonal k, and |k|
void diag_offsets(int64_t k, int64_t &r0, int64_t &c0) {
    GB_REQUIRE(k > -(1LL << 60) && k < (1LL << 60), GrB_INVALID_VALUE, "diagonal out of range");
    r0 = k < 0 ? -k : 0;
    c0 = k > 0 ? k : 0;
}

// C (n x n, n = size + |k|) = the diagonal matrix of v, cast to C's type
void matrix_diag(GB_Obj *C, GB_Obj *v, int64_t k) {
    int64_t r0, c0;
    diag_offsets(k, r0, c0);
    GB_REQUIRE(v->kind != GB_KIND_MATRIX || v->ncols == 1, GrB_DIMENSION_MISMATCH, "v must be a vector");
    const int64_t n = v->nrows + r0 + c0;
    GB_REQUIRE(C->nrows == n && gb_ncols_of(C) == n, GrB_DIMENSION_MISMATCH,
               "C must be n x n with n = the vector's size + |k|");
    gb_bitmap_view u;
    gb_get_bitmap(u, v);
    gb_mat_result T = bitmap_csr(u, true, n, n, r0, c0);
    cast_result(T, C->type->code);
    gb_install_csr(C, n, n, T.nvals, T.rowptr, T.colidx, T.vals, T.iso);
}

// w = diagonal k of A (of A' when tran: diagonal -k of A), cast to w's type
void vector_diag(GB_Obj *w, GB_Obj *A, int64_t k, bool tran) {
    if (tran) k = k == INT64_MIN ? INT64_MAX : -k;
    gb_csr_view v;
    gb_get_csr(v, A);
    int64_t size;  // any k is legal: a diagonal outside the matrix has no positions
    if (k >= 0) size = k >= v.ncols ? 0 : std::min(v.ncols - k, v.nrows);
    else size = k <= -v.nrows ? 0 : std::min(v.nrows + k, v.ncols);
    GB_REQUIRE(w->nrows == size && gb_ncols_of(w) == 1, GrB_DIMENSION_MISMATCH,
               "the output's size must be the length of the diagonal");
    const int64_t r0 = size && k < 0 ? -k : 0, c0 = size && k > 0 ? k : 0;
    const int wcode = w->type->code;
    const bool iso = v.iso && v.nvals > 0;
    gb_vec_result T = gb_new_vec_result(size, v.tcode, iso);
    gb_free(T.d_nvals);  // recounted by the install
    T.d_nvals = nullptr;
    const int64_t nw = gb_words(size);
    if (nw == 0) gb_memset(T.bits, 0, sizeof(uint64_t));
    if (iso) gb_copy_d2d(T.dense, v.vals, gb_type_size(v.tcode));
    const bool cast = wcode != v.tcode;
    if (cast && !iso && size) gb_memset(T.dense, 0, size * gb_type_size(v.tcode));  // the cast reads every position
    if (nw) {
        gb_with_size(gb_type_size(v.tcode), [&](auto x) {
            using W = decltype(x);
            hipLaunchKernelGGL((k_csr_diag<W>), dim3(gb_grid(nw, RIX_BLOCK / 64, RIX_GRID_CAP)), dim3(RIX_BLOCK), 0,
                               gb_stream(), size, r0, c0, v.rowptr, v.colidx, iso ? (const W *)nullptr : (const W *)v.vals,
                               T.bits, (W *)T.dense);
        });
        GB_LAUNCH_CHECK();
    }
    if (cast) {
        const int64_t nd = iso || size < 1 ? 1 : size;
        void *d = gb_malloc(nd * gb_type_size(wcode));
        if (iso || size) gb_cast_array(d, wcode, T.dense, v.tcode, nd);
        gb_free(T.dense);
        T.dense = d;
    }
    gb_install_bitmap(w, size, T.bits, T.dense, iso, nullptr);
}

// row pointer and columns of the row-major reshape of v (nvals > 0) into nr x nc
void reshape_rowmajor(const gb_csr_view &v, int64_t nr, int64_t nc, bool wide, int64_t **orp, int32_t **oci) {
    int64_t *rp = gb_malloc_n<int64_t>(nr + 1);
    int32_t *ci = nullptr;
    try {
        ci = gb_malloc_n<int32_t>(v.nvals);
    } catch (...) {
        gb_free(rp);
        throw;
    }
    const unsigned rgrid = gb_grid(nr + 1, RIX_BLOCK, RIX_GRID_CAP), cgrid = chunk_grid(v.nvals);
    auto go = [&](auto ix) {
        using IX = decltype(ix);
        hipLaunchKernelGGL((k_reshape_rowptr<IX>), dim3(rgrid), dim3(RIX_BLOCK), 0, gb_stream(), nr, v.nvals,
                           (IX)v.ncols, (IX)nc, v.rowptr, v.colidx, rp);
        hipLaunchKernelGGL((k_reshape_cols<IX>), dim3(cgrid), dim3(RIX_BLOCK), 0, gb_stream(), v.nvals, v.nrows,
                           (IX)v.ncols, (IX)nc, v.rowptr, v.colidx, ci);
    };
    try {
        if (wide) go(uint64_t{});
        else go(uint32_t{});
        GB_LAUNCH_CHECK();
    } catch (...) {
        gb_free(rp);
        gb_free(ci);
        throw;
    }
    *orp = rp;
    *oci = ci;
}

// what a reshape of an nrows x ncols object into nr x nc needs checked before anything changes;
// returns the number of positions
u128 reshape_check(int64_t nrows, int64_t ncols, GrB_Index nr, GrB_Index nc) {
    const u128 total = (u128)(uint64_t)nrows * (uint64_t)ncols;
    GB_REQUIRE((u128)nr * nc == total, GrB_DIMENSION_MISMATCH,
               "the new shape must hold as many positions as the old one");
    GB_REQUIRE(nr <= GrB_INDEX_MAX && nc <= GrB_INDEX_MAX, GrB_INVALID_VALUE, "dimension too large");
    // device column indices are int32, as in GrB_Matrix_new
    GB_REQUIRE(nc < (1ULL << 31), GrB_OUT_OF_MEMORY, "matrix with >= 2^31 columns exceeds the device index width");
    return total;
}

// the storage of the reshape of A into nr x nc (checked), in A's type.  keep_vals: a matrix A
// reshaped row-major keeps its value array, and T.vals comes back nullptr
gb_mat_result reshape_storage(GB_Obj *A, bool by_col, int64_t nr, int64_t nc, u128 total, bool keep_vals) {
    const bool wide = total > (u128)UINT32_MAX;
    gb_stat_set("reshape_div64", wide);
    const int tcode = A->type->code;
    const size_t ts = A->type->size;
    // column-major: the transposes carry the other dimension as int32 column indices
    const int64_t tr = by_col ? nc : nr, tc = by_col ? nr : nc;
    gb_mat_result T;
    if (A->kind != GB_KIND_MATRIX) {  // size x 1: both orders read the bitmap front to back
        gb_bitmap_view u;
        gb_get_bitmap(u, A);
        if (!A->dense) return gb_empty_mat_result(nr, nc, tcode);
        GB_REQUIRE(tc < (1LL << 31), GrB_NOT_IMPLEMENTED, "column-major reshape into 2^31 or more rows");
        T = bitmap_csr(u, false, tr, tc, 0, tc);
    } else {
        if (A->nvals == 0) return gb_empty_mat_result(nr, nc, tcode);
        GB_REQUIRE(total < ((u128)1 << 63), GrB_NOT_IMPLEMENTED, "reshape of more than 2^63 positions");
        GB_REQUIRE(!by_col || (A->nrows < (1LL << 31) && tc < (1LL << 31)), GrB_NOT_IMPLEMENTED,
                   "column-major reshape from or into 2^31 or more rows");
        gb_csr_view v;
        if (by_col) gb_get_csc(v, A);
        else gb_get_csr(v, A);
        T.nrows = tr;
        T.ncols = tc;
        T.nvals = v.nvals;
        T.iso = v.iso;
        T.tcode = tcode;
        reshape_rowmajor(v, tr, tc, wide, &T.rowptr, &T.colidx);
        if (!by_col && keep_vals) {
            T.vals = nullptr;
            return T;
        }
        if (by_col) {
            T.vals = const_cast<void *>(v.vals);  // the cached transpose's: read below, not owned
        } else {
            const int64_t nv = v.iso ? 1 : v.nvals;
            try {
                T.vals = gb_malloc(nv * ts);
            } catch (...) {
                gb_free(T.rowptr);
                gb_free(T.colidx);
                throw;
            }
            gb_copy_d2d(T.vals, v.vals, nv * ts);
        }
    }
    if (!by_col) return T;
    gb_mat_result R = T;
    R.nrows = nr;
    R.ncols = nc;
    auto release = [&] {  // the transposed intermediate; a matrix's values are its cached transpose's
        gb_free(T.rowptr);
        gb_free(T.colidx);
        if (A->kind != GB_KIND_MATRIX) gb_free(T.vals);
    };
    try {
        gb_transpose_csr(tr, tc, T.nvals, T.rowptr, T.colidx, T.vals, ts, T.iso, &R.rowptr, &R.colidx, &R.vals);
    } catch (...) {
        release();
        throw;
    }
    release();
    return R;
}

// w(lin) = A(i, j), cast to w's type
void vector_flatten(GB_Obj *w, GB_Obj *A, bool by_col) {
    gb_csr_view v;
    gb_get_csr(v, A);
    const u128 total = (u128)(uint64_t)v.nrows * (uint64_t)v.ncols;
    GB_REQUIRE(total == (u128)(uint64_t)w->nrows && gb_ncols_of(w) == 1, GrB_DIMENSION_MISMATCH,
               "the output's size must be nrows * ncols");
    const int64_t n = w->nrows, nw = gb_words(n);
    const int wcode = w->type->code;
    const bool iso = v.iso && v.nvals > 0;
    gb_vec_result T = gb_new_vec_result(n, wcode, iso);
    gb_free(T.d_nvals);  // recounted by the install
    T.d_nvals = nullptr;
    gb_memset(T.bits, 0, (nw ? nw : 1) * sizeof(uint64_t));
    gb_scratch s;
    const void *vx = v.nvals ? gb_view_vals_as(v, wcode, s) : nullptr;
    if (iso) gb_copy_d2d(T.dense, vx, gb_type_size(wcode));
    if (v.nvals) {
        gb_with_size(gb_type_size(wcode), [&](auto x) {
            using W = decltype(x);
            hipLaunchKernelGGL((k_flatten<W>), dim3(chunk_grid(v.nvals)), dim3(RIX_BLOCK), 0, gb_stream(), v.nvals,
                               v.nrows, by_col ? (int64_t)1 : v.ncols, by_col ? v.nrows : (int64_t)1, v.rowptr,
                               v.colidx, iso ? (const W *)nullptr : (const W *)vx, (unsigned long long *)T.bits,
                               (W *)T.dense);
        });
        GB_LAUNCH_CHECK();
    }
    gb_install_bitmap(w, n, T.bits, T.dense, iso, nullptr);
}

// ---- dense import / export.  Layout: A(i, j) sits at X[i * ncols + j]; by_col (X[i + j * nrows])
// is the row-major array of the transpose, so the import ends in gb_transpose_csr and the export
// reads gb_get_csc's view: no strided access.  A dense array is a full bitmap in position order
// once k_dense_flags has decided which positions hold entries, and bitmap_csr does the rest.

// a GrB_Scalar argument read on the host and cast to type `code`: present = it holds a value
struct dense_scalar {
    bool present = false;
    alignas(8) unsigned char bytes[8] = {};
    template <class W>
    W as() const {
        W w;
        memcpy(&w, bytes, sizeof(W));
        return w;
    }
};

GrB_Info read_dense_scalar(dense_scalar &v, const GrB_Scalar s, int code) {
    if (!s) return GrB_SUCCESS;
    GB_Obj *S = OBJ(s);
    if (S->magic != GB_MAGIC) return GrB_UNINITIALIZED_OBJECT;
    alignas(8) unsigned char own[8] = {};
    GrB_Info r = GrB_DOMAIN_MISMATCH;
    switch (S->type->code) {
#define GB_READ(T, ctype)                                                 \
    case GBAMD_T_##T:                                                     \
        r = GrB_Scalar_extractElement_##T((ctype *)own, s);               \
        break;
        GB_FOR_EACH_TYPE(GB_READ)
#undef GB_READ
    }
    if (r == GrB_NO_VALUE) return GrB_SUCCESS;
    if (r != GrB_SUCCESS) return r;
    gb_cast_scalar(v.bytes, code, own, S->type->code);
    v.present = true;
    return GrB_SUCCESS;
}

// what GrB_Matrix_new checks of a shape (both dimensions as columns, when the transpose is
// built); returns the number of positions
int64_t dense_positions(GrB_Index nrows, GrB_Index ncols, bool both) {
    GB_REQUIRE(nrows <= GrB_INDEX_MAX && ncols <= GrB_INDEX_MAX, GrB_INVALID_VALUE, "dimension too large");
    GB_REQUIRE(ncols < (1ULL << 31) && (!both || nrows < (1ULL << 31)), GrB_OUT_OF_MEMORY,
               "matrix with >= 2^31 columns exceeds the device index width");
    const u128 total = (u128)nrows * ncols;
    GB_REQUIRE(total < ((u128)1 << 63), GrB_OUT_OF_MEMORY, "dense array of 2^63 or more positions");
    return (int64_t)total;
}

// a host array's device copy, or the device array itself
const void *dense_stage_in(const void *p, size_t bytes, bool on_device, gb_scratch &s) {
    if (on_device || !p) return p;
    char *d = s.get<char>(bytes);
    gb_copy_h2d(d, p, bytes);
    return d;
}

// bits (nw words, nw >= 1) = which of the n positions of X / Ab (device) hold an entry
void dense_flags(int64_t n, int code, const void *X, const int8_t *Ab, const dense_scalar &m, uint64_t *bits) {
    auto go = [&](auto c) {
        using C = decltype(c);
        hipLaunchKernelGGL((k_dense_flags<C>), dim3(chunk_grid(n)), dim3(RIX_BLOCK), 0, gb_stream(), n, (const C *)X,
                           Ab, m.present, m.as<C>(), bits);
    };
    if (!m.present) go(uint8_t());  // X is not read
    else if (code == GBAMD_T_FP32) go(float());
    else if (code == GBAMD_T_FP64) go(double());
    else gb_with_size(gb_type_size(code), go);
    GB_LAUNCH_CHECK();
}

// the CSR of nrows x ncols of the dense array X / Ab (device pointers), in X's type
gb_mat_result dense_to_csr(int code, int64_t nrows, int64_t ncols, int64_t n, const void *X, const int8_t *Ab,
                           const dense_scalar &m, bool by_col) {
    gb_stat_set("reshape_div64", n > (int64_t)UINT32_MAX);
    if (n == 0) return gb_empty_mat_result(nrows, ncols, code);
    const int64_t tr = by_col ? ncols : nrows, tc = by_col ? nrows : ncols;
    gb_scratch s;
    uint64_t *bits = s.get<uint64_t>(gb_words(n));
    dense_flags(n, code, X, Ab, m, bits);
    gb_bitmap_view u;
    u.n = n;
    u.bits = bits;
    u.vals = X;
    u.tcode = code;
    gb_mat_result T = bitmap_csr(u, false, tr, tc, 0, tc);
    if (!by_col) return T;
    auto release = [&] {
        gb_free(T.rowptr);
        gb_free(T.colidx);
        gb_free(T.vals);
    };
    gb_mat_result R = T;
    R.nrows = nrows;
    R.ncols = ncols;
    try {
        if (T.nvals == 0) R = gb_empty_mat_result(nrows, ncols, code);
        else
            gb_transpose_csr(tr, tc, T.nvals, T.rowptr, T.colidx, T.vals, gb_type_size(code), false, &R.rowptr,
                             &R.colidx, &R.vals);
    } catch (...) {
        release();
        throw;
    }
    release();
    return R;
}

void fill_array(int64_t n, size_t ts, void *X, const dense_scalar &fill) {
    gb_with_size(ts, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((k_dense_fill<W>), dim3(chunk_grid(n * (int64_t)sizeof(W) / 16)), dim3(RIX_BLOCK), 0,
                           gb_stream(), n, (W *)X, fill.as<W>());
    });
    GB_LAUNCH_CHECK();
}

// X / Ab (device, n positions) = the dense array of A, row-major, or of A' when by_col
void csr_to_dense(GB_Obj *A, bool by_col, int64_t n, void *X, int8_t *Ab, const dense_scalar &fill) {
    gb_csr_view v;
    if (by_col) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    const size_t ts = A->type->size;
    if (v.nvals < n) {
        fill_array(n, ts, X, fill);
        if (Ab) fill_array(n, 1, Ab, dense_scalar());
    }
    if (v.nvals == 0) return;
    gb_with_size(ts, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((k_dense_scatter<W>), dim3(chunk_grid(v.nvals)), dim3(RIX_BLOCK), 0, gb_stream(), v.nvals,
                           v.nrows, v.ncols, v.rowptr, v.colidx, (const W *)v.vals, v.iso, (W *)X, Ab);
    });
    GB_LAUNCH_CHECK();
}

// the export of both kinds: A as nrows x ncols (a vector: size x 1, read off its bitmap)
void export_dense(void *X, int8_t *Ab, GB_Obj *A, const dense_scalar &fill, bool by_col, bool on_device) {
    const bool bitmap = A->kind != GB_KIND_MATRIX;
    const u128 total = (u128)(uint64_t)A->nrows * (uint64_t)gb_ncols_of(A);
    GB_REQUIRE(total < ((u128)1 << 63), GrB_OUT_OF_MEMORY, "dense array of 2^63 or more positions");
    const int64_t n = (int64_t)total;
    if (n == 0) return;
    GB_REQUIRE(X, GrB_NULL_POINTER, "X is NULL");
    GB_REQUIRE(fill.present || Ab || gb_nvals(A) == n, GrB_INVALID_VALUE,
               "a fill value or a bitmap is needed when there are missing values");
    const size_t ts = A->type->size;
    gb_scratch s;
    void *dX = on_device ? X : s.get<char>(n * ts);
    int8_t *dAb = on_device || !Ab ? Ab : s.get<int8_t>(n);
    if (bitmap) {
        gb_bitmap_view u;
        gb_get_bitmap(u, A);
        gb_with_size(ts, [&](auto w) {
            using W = decltype(w);
            hipLaunchKernelGGL((k_bitmap_dense<W>), dim3(chunk_grid(n)), dim3(RIX_BLOCK), 0, gb_stream(), n, u.bits,
                               (const W *)u.vals, u.iso, fill.as<W>(), (W *)dX, dAb);
        });
        GB_LAUNCH_CHECK();
    } else {
        csr_to_dense(A, by_col, n, dX, dAb, fill);
    }
    if (on_device) return;
    gb_copy_d2h(X, dX, n * ts);
    if (Ab) gb_copy_d2h(Ab, dAb, n);
}

}  // namespace

extern "C" {

GrB_Info GxB_Matrix_import_dense(GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void *X,
                                 const int8_t *Ab, const GrB_Scalar missing, bool by_col, bool on_device) {
    if (!A) return GrB_NULL_POINTER;
    if (!type || type->magic != GB_MAGIC) return GrB_UNINITIALIZED_OBJECT;
    dense_scalar m;
    GrB_Info e = read_dense_scalar(m, missing, type->code);
    if (e != GrB_SUCCESS) return e;
    return gb_api(nullptr, [&] {
        const int64_t n = dense_positions(nrows, ncols, by_col);
        GB_REQUIRE(X || n == 0, GrB_NULL_POINTER, "X is NULL");
        const int64_t nr = (int64_t)nrows, nc = (int64_t)ncols;
        GB_Obj *Ao = gb_new_object_bare(GB_KIND_MATRIX, type, nr, nc);
        try {
            gb_scratch s;
            const void *dX = dense_stage_in(X, n * type->size, on_device, s);
            const int8_t *dAb = (const int8_t *)dense_stage_in(Ab, n, on_device, s);
            gb_mat_result T = dense_to_csr(type->code, nr, nc, n, dX, dAb, m, by_col);
            gb_install_csr(Ao, nr, nc, T.nvals, T.rowptr, T.colidx, T.vals, false);
        } catch (...) {
            free_bare(Ao);
            throw;
        }
        *A = (GrB_Matrix)Ao;
    });
}

GrB_Info GxB_Vector_import_dense(GrB_Vector *v, GrB_Type type, GrB_Index n, const void *X, const int8_t *Ab,
                                 const GrB_Scalar missing, bool on_device) {
    if (!v) return GrB_NULL_POINTER;
    if (!type || type->magic != GB_MAGIC) return GrB_UNINITIALIZED_OBJECT;
    dense_scalar m;
    GrB_Info e = read_dense_scalar(m, missing, type->code);
    if (e != GrB_SUCCESS) return e;
    return gb_api(nullptr, [&] {
        GB_REQUIRE(n <= GrB_INDEX_MAX, GrB_INVALID_VALUE, "dimension too large");
        GB_REQUIRE(X || n == 0, GrB_NULL_POINTER, "X is NULL");
        const int64_t size = (int64_t)n;
        GB_Obj *vo = gb_new_object_bare(GB_KIND_VECTOR, type, size, 1);
        try {
            gb_vec_result T = gb_new_vec_result(size, type->code, false);
            gb_free(T.d_nvals);  // recounted by the install
            T.d_nvals = nullptr;
            try {
                if (size == 0) {
                    gb_memset(T.bits, 0, sizeof(uint64_t));
                } else {
                    // the values are one copy; the words are the object's bitmap
                    if (on_device) gb_copy_d2d(T.dense, X, size * type->size);
                    else gb_copy_h2d(T.dense, X, size * type->size);
                    gb_scratch s;
                    const int8_t *dAb = (const int8_t *)dense_stage_in(Ab, size, on_device, s);
                    dense_flags(size, type->code, T.dense, dAb, m, T.bits);
                }
            } catch (...) {
                gb_free(T.bits);
                gb_free(T.dense);
                throw;
            }
            gb_install_bitmap(vo, size, T.bits, T.dense, false, nullptr);
        } catch (...) {
            free_bare(vo);
            throw;
        }
        *v = (GrB_Vector)vo;
    });
}

GrB_Info GxB_Matrix_export_dense(void *X, int8_t *Ab, const GrB_Matrix A, const GrB_Scalar fill, bool by_col,
                                 bool on_device) {
    if (!A) return GrB_NULL_POINTER;
    if (OBJ(A)->magic != GB_MAGIC) return GrB_UNINITIALIZED_OBJECT;
    dense_scalar f;
    GrB_Info e = read_dense_scalar(f, fill, OBJ(A)->type->code);
    if (e != GrB_SUCCESS) return e;
    return gb_api(OBJ(A), [&] { export_dense(X, Ab, gb_obj_check(A), f, by_col, on_device); });
}

GrB_Info GxB_Vector_export_dense(void *X, int8_t *Ab, const GrB_Vector v, const GrB_Scalar fill, bool on_device) {
    return GxB_Matrix_export_dense(X, Ab, (GrB_Matrix)v, fill, false, on_device);
}

GrB_Info GrB_Matrix_diag(GrB_Matrix *C, const GrB_Vector v, int64_t k) {
    if (!C) return GrB_NULL_POINTER;
    return gb_api(nullptr, [&] {
        GB_Obj *vo = gb_obj_check(v);
        int64_t r0, c0;
        diag_offsets(k, r0, c0);
        const int64_t n = vo->nrows + r0 + c0;
        GB_Obj *Co = gb_new_object_bare(GB_KIND_MATRIX, vo->type, n, n);
        try {
            matrix_diag(Co, vo, k);
        } catch (...) {
            free_bare(Co);
            throw;
        }
        *C = (GrB_Matrix)Co;
    });
}

GrB_Info GxB_Matrix_diag(GrB_Matrix C, const GrB_Vector v, int64_t k, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C);
        GB_Obj *vo = gb_obj_check(v);
        gb_read_desc(desc);
        matrix_diag(Co, vo, k);
    });
}

GrB_Info GxB_Vector_diag(GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc) {
    return gb_api(OBJ(v), [&] {
        GB_Obj *vo = gb_obj_check(v);
        GB_Obj *Ao = gb_obj_check(A);
        vector_diag(vo, Ao, k, gb_read_desc(desc).tran0);
    });
}

GrB_Info GxB_Matrix_reshape(GrB_Matrix C, bool by_col, GrB_Index nrows_new, GrB_Index ncols_new,
                            const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C);
        gb_read_desc(desc);
        const u128 total = reshape_check(Co->nrows, gb_ncols_of(Co), nrows_new, ncols_new);
        if (Co->kind != GB_KIND_MATRIX) {
            GB_REQUIRE(ncols_new == 1, GrB_INVALID_VALUE, "a vector keeps its one column");
            return;
        }
        const int64_t nr = (int64_t)nrows_new, nc = (int64_t)ncols_new;
        gb_mat_result T = reshape_storage(Co, by_col, nr, nc, total, true);
        if (!T.vals) {  // row-major with entries: the value array stays where it is
            T.vals = Co->vals;
            Co->vals = nullptr;
        }
        gb_install_csr(Co, nr, nc, T.nvals, T.rowptr, T.colidx, T.vals, T.iso);
    });
}

GrB_Info GxB_Matrix_reshapeDup(GrB_Matrix *C, GrB_Matrix A, bool by_col, GrB_Index nrows_new, GrB_Index ncols_new,
                               const GrB_Descriptor desc) {
    if (!C) return GrB_NULL_POINTER;
    return gb_api(OBJ(A), [&] {
        GB_Obj *Ao = gb_obj_check(A);
        gb_read_desc(desc);
        const u128 total = reshape_check(Ao->nrows, gb_ncols_of(Ao), nrows_new, ncols_new);
        const int64_t nr = (int64_t)nrows_new, nc = (int64_t)ncols_new;
        GB_Obj *Co = gb_new_object_bare(GB_KIND_MATRIX, Ao->type, nr, nc);
        try {
            gb_mat_result T = reshape_storage(Ao, by_col, nr, nc, total, false);
            gb_install_csr(Co, nr, nc, T.nvals, T.rowptr, T.colidx, T.vals, T.iso);
        } catch (...) {
            free_bare(Co);
            throw;
        }
        *C = (GrB_Matrix)Co;
    });
}

GrB_Info GxB_Vector_flatten(GrB_Vector w, const GrB_Matrix A, bool by_col, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_Obj *wo = gb_obj_check(w);
        GB_Obj *Ao = gb_obj_check(A);
        gb_read_desc(desc);
        vector_flatten(wo, Ao, by_col);
    });
}

}  // extern "C"
