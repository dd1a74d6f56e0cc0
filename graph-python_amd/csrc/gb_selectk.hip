// gb_selectk.hip -- GxB_{Matrix,Vector}_selectk / _compactify: k entries of every row.
//   reference core/ss/matrix.py:3815-3989, core/ss/vector.py:1407-1560
//
// A row's d entries have positions 0 .. d-1 (ascending column).  `how` orders them: FIRST by
// position, LAST reversed, SMALLEST ascending by (sort key, position) -- the order of
// GxB_Matrix_sort under GrB_LT --, LARGEST that reversed, RANDOM ascending by
// (gb_hash3(seed, row, position), position).  selectk keeps the first min(k, d) of that order in
// place, compactify moves them to columns 0 .. min(k, d)-1 (their values, or their columns).
//
// The output row pointer is a closed form, the scan of min(k, d): nothing is counted after the
// selection, and every kernel below writes to its final place.
//   FIRST / LAST      one entry-parallel gather over the output entries (k_selk_gather): output
//                     entry t of row i comes from rp[i] + u or rp[i+1] - 1 - u.
//   SMALLEST / LARGEST / RANDOM
//     compactify      the sort's row classes (gb_rank_rows, gb_sort.hip) with a trimmed emit:
//                     only ranks below min(k, d) are written, from the far end for LARGEST.
//     selectk, and compactify RANDOM (which emits in ascending position)
//                     the same classes over the rows of more than k entries only, marking the
//                     chosen entries in a byte per entry; k_selk_whole adds the rows kept whole,
//                     a scan of the bytes gives every kept entry its place (the same closed-form
//                     row pointer), and k_selk_scatter moves it there.  Random keys are computed
//                     where they are compared and stored for the long rows only.
// Columnwise: the rows of the cached CSC, and the result back to CSR through gb_transpose_csr.
// An iso A: SMALLEST and LARGEST are FIRST (as in the reference); compactify without asindex
// moves no values at all.
//
// Vectors: gb_bitmap_order (the vector sort's compaction, key build and gb_sort_pairs_u64) lists
// the entries in the order of `how`; selectk marks the first min(k, nvals) of the list in a
// bitmap, compactify copies them out (RANDOM: through that bitmap, listed again by index).
#include <algorithm>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SELK_BLOCK 256
#define SELK_WPI 4  // a wave takes chunks of SELK_WPI * 64 entries
#define SELK_WAVE_CAP 64
#define SELK_BLOCK_CAP 2048

namespace {

enum { HOW_FIRST = 0, HOW_LAST, HOW_SMALLEST, HOW_LARGEST, HOW_RANDOM };

// of the last matrix call, on the device: [0..3] the ranking's rows per class as the sort counts
// them (wave, workgroup of one wave, long, workgroup of 256), [4] rows of at most k entries
unsigned long long *g_selk_stats = nullptr;

int selk_knob(const char *key, int dflt) {
    const int64_t k = gb_knob(key);
    return k > 0 && k < dflt ? (int)k : dflt;
}

GB_DEV void selk_move(void *dst, int64_t q, const void *src, int64_t p, int vs) {
    switch (vs) {
    case 1: ((uint8_t *)dst)[q] = ((const uint8_t *)src)[p]; break;
    case 2: ((uint16_t *)dst)[q] = ((const uint16_t *)src)[p]; break;
    case 4: ((uint32_t *)dst)[q] = ((const uint32_t *)src)[p]; break;
    default: ((uint64_t *)dst)[q] = ((const uint64_t *)src)[p]; break;
    }
}

GB_DEV void selk_zero(void *dst, int64_t q, int vs) {
    switch (vs) {
    case 1: ((uint8_t *)dst)[q] = 0; break;
    case 2: ((uint16_t *)dst)[q] = 0; break;
    case 4: ((uint32_t *)dst)[q] = 0; break;
    default: ((uint64_t *)dst)[q] = 0; break;
    }
}

// len[i] = min(k, d_i); *whole += rows with d_i <= k; *longest = max d_i (either may be null)
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_lens(int64_t nrows, const int64_t *__restrict__ rp, int64_t k,
                                                          int64_t *__restrict__ len, unsigned long long *whole,
                                                          unsigned long long *longest) {
    const int lane = threadIdx.x & 63;
    unsigned long long mx = 0;
    const int64_t stride = (int64_t)gridDim.x * SELK_BLOCK;
    for (int64_t base = blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x - lane; base < nrows; base += stride) {
        const int64_t i = base + lane;
        int64_t d = -1;
        if (i < nrows) {
            d = rp[i + 1] - rp[i];
            if (len) len[i] = d < k ? d : k;
            if ((unsigned long long)d > mx) mx = (unsigned long long)d;
        }
        const unsigned long long b = __ballot(d >= 0 && d <= k);
        if (whole && b && lane == 0) atomicAdd(whole, (unsigned long long)__popcll(b));
    }
    if (longest) {
        for (int j = 32; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(mx, j);
            if (o > mx) mx = o;
        }
        if (lane == 0 && mx) atomicMax(longest, mx);
    }
}

struct selk_out {
    int64_t nrows, onv;
    const int64_t *rp;      // input rows
    const int32_t *ci;
    const void *avals;
    int vs;                 // bytes of a value
    const int64_t *orp;     // output rows
    int32_t *ocol;
    void *oC;               // values (nullptr: iso, none moved)
    uint64_t *oI;           // the entries' columns as values (asindex)
    bool compact;           // the output column is the slot, not the entry's own
};

// FIRST / LAST: output entry t of row i (m entries) is u = rev ? m-1-t : t of the order, which is
// input entry rp[i] + u, or rp[i+1] - 1 - u from the end
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_gather(selk_out o, bool last, bool rev) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * SELK_BLOCK) >> 6;
    const int64_t nchunks = (o.onv + SELK_WPI * 64 - 1) / (SELK_WPI * 64);
    int64_t next = -1;
    for (int64_t c = wave; c < nchunks; c += nwaves) {
        int64_t row[SELK_WPI];
        const int64_t q0 = c * (SELK_WPI * 64);
        gb_chunk_rows<SELK_WPI>(o.orp, o.nrows, o.onv, q0, lane, next, row);
#pragma unroll
        for (int w = 0; w < SELK_WPI; w++) {
            const int64_t q = q0 + w * 64 + lane;
            if (q >= o.onv) continue;
            const int64_t i = row[w], os = o.orp[i], t = q - os, m = o.orp[i + 1] - os;
            const int64_t u = rev ? m - 1 - t : t;
            const int64_t p = last ? o.rp[i + 1] - 1 - u : o.rp[i] + u;
            o.ocol[q] = o.compact ? (int32_t)t : o.ci[p];
            if (o.oI) o.oI[q] = (uint64_t)o.ci[p];
            if (o.oC) selk_move(o.oC, q, o.avals, p, o.vs);
        }
    }
}

// keep[p] = 1 for every entry of a row of at most k entries (the ranking skipped those rows)
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_whole(int64_t nrows, int64_t nvals, const int64_t *__restrict__ rp,
                                                           int64_t k, uint8_t *__restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * SELK_BLOCK) >> 6;
    const int64_t nchunks = (nvals + SELK_WPI * 64 - 1) / (SELK_WPI * 64);
    int64_t next = -1;
    for (int64_t c = wave; c < nchunks; c += nwaves) {
        int64_t row[SELK_WPI];
        const int64_t p0 = c * (SELK_WPI * 64);
        gb_chunk_rows<SELK_WPI>(rp, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int w = 0; w < SELK_WPI; w++) {
            const int64_t p = p0 + w * 64 + lane;
            if (p >= nvals) continue;
            const int64_t i = row[w];
            if (rp[i + 1] - rp[i] <= k) keep[p] = 1;
        }
    }
}

// every kept input entry p to its place pos[p] (the exclusive scan of keep)
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_scatter(selk_out o, int64_t nvals, const uint8_t *__restrict__ keep,
                                                             const int64_t *__restrict__ pos) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * SELK_BLOCK) >> 6;
    const int64_t nchunks = (nvals + SELK_WPI * 64 - 1) / (SELK_WPI * 64);
    int64_t next = -1;
    for (int64_t c = wave; c < nchunks; c += nwaves) {
        int64_t row[SELK_WPI];
        const int64_t p0 = c * (SELK_WPI * 64);
        if (o.compact) gb_chunk_rows<SELK_WPI>(o.rp, o.nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int w = 0; w < SELK_WPI; w++) {
            const int64_t p = p0 + w * 64 + lane;
            if (p >= nvals || !keep[p]) continue;
            const int64_t q = pos[p];
            if (q >= o.onv) continue;  // cannot be: the scan and the row pointer count the same entries
            o.ocol[q] = o.compact ? (int32_t)(q - o.orp[row[w]]) : o.ci[p];
            if (o.oI) o.oI[q] = (uint64_t)o.ci[p];
            if (o.oC) selk_move(o.oC, q, o.avals, p, o.vs);
        }
    }
}

int64_t clamp_k(GrB_Index k) { return k > (GrB_Index)(1LL << 62) ? (1LL << 62) : (int64_t)k; }

void check_how(int how) {
    GB_REQUIRE(how >= HOW_FIRST && how <= HOW_RANDOM, GrB_INVALID_VALUE, "how is not a GxB_SelectK_How");
}

void check_type(GB_Obj *C, int tcode, bool asindex) {
    GB_REQUIRE(C->type->code == tcode || (asindex && C->type->code == GBAMD_T_UINT64), GrB_DOMAIN_MISMATCH,
               asindex ? "the output must have A's type or GrB_UINT64" : "the output must have A's type");
}

void matrix_selectk(GB_Obj *C, GB_Obj *A, int how, int64_t k, bool compact, bool reverse, bool asindex, uint64_t seed,
                    const gb_desc &d) {
    check_how(how);
    GB_REQUIRE(A->kind == GB_KIND_MATRIX && C->kind == GB_KIND_MATRIX, GrB_INVALID_OBJECT, "not a matrix");
    if (!compact) {
        reverse = asindex = false;
        GB_REQUIRE(C->nrows == A->nrows && C->ncols == A->ncols, GrB_DIMENSION_MISMATCH,
                   "output dimensions do not match A");
    } else if (d.tran0) {
        GB_REQUIRE(C->nrows == k && C->ncols == A->ncols, GrB_DIMENSION_MISMATCH, "the output is not k x ncols(A)");
    } else {
        GB_REQUIRE(C->nrows == A->nrows && C->ncols == k, GrB_DIMENSION_MISMATCH, "the output is not nrows(A) x k");
    }
    check_type(C, A->type->code, asindex);
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    const int64_t nr = v.nrows, nv = v.nvals;
    const size_t vs = gb_type_size(v.tcode);
    if (v.iso) {  // equal values: nothing to compare, and without asindex nothing to tell apart
        if (how == HOW_SMALLEST || how == HOW_LARGEST || (how == HOW_RANDOM && compact && !asindex)) {
            how = HOW_FIRST;
            if (compact) reverse = false;
        }
    }
    if (how == HOW_RANDOM) reverse = false;
    if (!g_selk_stats) g_selk_stats = gb_malloc_n<unsigned long long>(5);
    gb_memset(g_selk_stats, 0, 5 * sizeof(unsigned long long));
    const gb_desc d0;
    if (nv == 0 || k == 0) {  // nothing is kept
        gb_mat_result E = gb_empty_mat_result(C->nrows, C->ncols, asindex ? GBAMD_T_UINT64 : v.tcode);
        gb_writeback_matrix(C, E, nullptr, d0, nullptr);
        return;
    }

    gb_mat_result T;
    T.nrows = nr;
    T.ncols = compact ? k : v.ncols;
    T.tcode = asindex ? GBAMD_T_UINT64 : v.tcode;
    T.iso = v.iso && !asindex;
    const size_t os = asindex ? sizeof(uint64_t) : vs;
    // the output row pointer: the scan of min(k, d)
    T.rowptr = gb_malloc_n<int64_t>(nr + 1);
    {
        gb_scratch s;
        int64_t *len = s.get<int64_t>(nr);
        hipLaunchKernelGGL(k_selk_lens, dim3(gb_sort_grid(nr, SELK_BLOCK)), dim3(SELK_BLOCK), 0, gb_stream(), nr,
                           v.rowptr, k, len, g_selk_stats + 4, (unsigned long long *)nullptr);
        GB_LAUNCH_CHECK();
        gb_exclusive_scan_i64(len, T.rowptr, nr);
    }
    const int64_t onv = gb_read_i64(T.rowptr + nr);
    T.nvals = onv;
    T.colidx = gb_malloc_n<int32_t>(onv < 1 ? 1 : onv);
    T.vals = gb_malloc((T.iso || onv < 1 ? 1 : onv) * os);
    if (T.iso) gb_copy_d2d(T.vals, v.vals, vs);
    if (onv > 0) {
        selk_out o{};
        o.nrows = nr;
        o.onv = onv;
        o.rp = v.rowptr;
        o.ci = v.colidx;
        o.avals = v.vals;
        o.vs = (int)vs;
        o.orp = T.rowptr;
        o.ocol = T.colidx;
        o.oC = asindex || T.iso ? nullptr : T.vals;
        o.oI = asindex ? (uint64_t *)T.vals : nullptr;
        o.compact = compact;
        const unsigned ogrid = gb_sort_grid((onv + SELK_WPI * 64 - 1) / (SELK_WPI * 64), SELK_BLOCK / 64);
        const unsigned igrid = gb_sort_grid((nv + SELK_WPI * 64 - 1) / (SELK_WPI * 64), SELK_BLOCK / 64);
        if (how == HOW_FIRST || how == HOW_LAST) {
            // selectk keeps the entries in column order: LAST's kept run, read backwards from the end
            const bool rev = compact ? reverse : how == HOW_LAST;
            hipLaunchKernelGGL(k_selk_gather, dim3(ogrid), dim3(SELK_BLOCK), 0, gb_stream(), o, how == HOW_LAST, rev);
            GB_LAUNCH_CHECK();
        } else {
            gb_scratch s;
            gb_rank_job j;
            j.nrows = nr;
            j.nvals = nv;
            j.rowptr = v.rowptr;
            j.colidx = v.colidx;
            j.random = how == HOW_RANDOM;
            j.seed = seed;
            j.xin = v.vals;  // compared as A's own type (an iso A never comes here by value)
            j.xcode = v.tcode;
            j.avals = v.vals;
            j.vs = (int)vs;
            j.m = k;
            j.far = how == HOW_LARGEST;
            j.orp = T.rowptr;
            j.wave_max = selk_knob("selectk_wave_max", SELK_WAVE_CAP);
            j.block_max = selk_knob("selectk_block_max", SELK_BLOCK_CAP);
            j.stats = g_selk_stats;
            if (compact && how != HOW_RANDOM) {
                j.reverse = reverse;
                j.oC = o.oC;
                j.oP = (int64_t *)o.oI;
                j.ocol = T.colidx;
                gb_rank_rows(j);
            } else {
                uint8_t *keep = s.get<uint8_t>(nv);
                int64_t *pos = s.get<int64_t>(nv + 1);
                gb_memset(keep, 0, nv);
                j.keep = keep;
                gb_rank_rows(j);
                hipLaunchKernelGGL(k_selk_whole, dim3(igrid), dim3(SELK_BLOCK), 0, gb_stream(), nr, nv, v.rowptr, k,
                                   keep);
                GB_LAUNCH_CHECK();
                gb_exclusive_scan_u8(keep, pos, nv);
                hipLaunchKernelGGL(k_selk_scatter, dim3(igrid), dim3(SELK_BLOCK), 0, gb_stream(), o, nv,
                                   (const uint8_t *)keep, (const int64_t *)pos);
                GB_LAUNCH_CHECK();
            }
        }
    }
    if (d.tran0) {  // back to CSR: T is (a selection of) A', or the compacted columns as rows
        gb_mat_result R;
        R.nrows = T.ncols;
        R.ncols = T.nrows;
        R.nvals = onv;
        R.tcode = T.tcode;
        R.iso = T.iso;
        gb_transpose_csr(T.nrows, T.ncols, onv, T.rowptr, T.colidx, T.vals, os, T.iso, &R.rowptr, &R.colidx, &R.vals);
        gb_free(T.rowptr);
        gb_free(T.colidx);
        gb_free(T.vals);
        T = R;
    }
    gb_writeback_matrix(C, T, nullptr, d0, nullptr);
}

// ------------------------------------------------------------------ vectors
// the first min(k, nvals) entries of the listed order (from the far end of the list if far)
// marked in keepbits (zeroed by the caller)
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_vec_mark(int64_t n, const int64_t *__restrict__ off,
                                                              const int64_t *__restrict__ idx, int64_t k, bool far,
                                                              unsigned long long *__restrict__ keepbits) {
    const int64_t nvals = off[(n + 63) >> 6];
    const int64_t m = k < nvals ? k : nvals;
    for (int64_t t = blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x; t < m; t += (int64_t)gridDim.x * SELK_BLOCK) {
        const int64_t i = idx[far ? nvals - 1 - t : t];
        atomicOr(&keepbits[i >> 6], 1ull << (i & 63));
    }
}

// selectk's result: the marked entries of u at their own indices
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_vec_select(int64_t n, const int64_t *__restrict__ off, int64_t k,
                                                                const uint64_t *__restrict__ keepbits,
                                                                const void *__restrict__ uvals, int vs, void *wvals,
                                                                uint64_t *__restrict__ wbits, int64_t *wcount) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t nvals = off[(n + 63) >> 6];
        *wcount = k < nvals ? k : nvals;
    }
    for (int64_t i = blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SELK_BLOCK) {
        const uint64_t b = keepbits[i >> 6];
        if ((i & 63) == 0) wbits[i >> 6] = b;
        if (wvals) {
            if ((b >> (i & 63)) & 1) selk_move(wvals, i, uvals, i, vs);
            else selk_zero(wvals, i, vs);
        }
    }
}

// compactify's result of size N: slot t < m = min(N, nvals) holds entry u = reverse ? m-1-t : t of the
// listed order (from the far end of the list if far): its value, or its index; zero beyond, and
// a bitmap of m ones
__global__ __launch_bounds__(SELK_BLOCK) void k_selk_vec_emit(int64_t N, int64_t n, const int64_t *__restrict__ off,
                                                              const int64_t *__restrict__ idx, bool far, bool reverse,
                                                              const void *__restrict__ uvals, int vs, void *wvals,
                                                              uint64_t *wI, uint64_t *__restrict__ wbits,
                                                              int64_t *wcount) {
    const int64_t nvals = off[(n + 63) >> 6];
    const int64_t m = N < nvals ? N : nvals;
    if (blockIdx.x == 0 && threadIdx.x == 0) *wcount = m;
    for (int64_t t = blockIdx.x * (int64_t)SELK_BLOCK + threadIdx.x; t < N; t += (int64_t)gridDim.x * SELK_BLOCK) {
        const bool real = t < m;
        const int64_t u = reverse ? m - 1 - t : t;
        const int64_t src = real ? idx[far ? nvals - 1 - u : u] : 0;
        if (wI) wI[t] = real ? (uint64_t)src : 0;
        if (wvals) {
            if (real) selk_move(wvals, t, uvals, src, vs);
            else selk_zero(wvals, t, vs);
        }
        if ((t & 63) == 0) {
            const int64_t left = m - t;
            wbits[t >> 6] = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0;
        }
    }
}

void vector_selectk(GB_Obj *W, GB_Obj *U, int how, int64_t k, bool compact, bool reverse, bool asindex, uint64_t seed) {
    check_how(how);
    GB_REQUIRE(gb_ncols_of(U) == 1 && gb_ncols_of(W) == 1, GrB_DIMENSION_MISMATCH, "not a vector");
    if (!compact) reverse = asindex = false;
    GB_REQUIRE(W->nrows == (compact ? k : U->nrows), GrB_DIMENSION_MISMATCH,
               compact ? "the output's size is not k" : "output size does not match u");
    check_type(W, U->type->code, asindex);
    gb_bitmap_view uv;
    gb_get_bitmap(uv, U);
    const int64_t n = uv.n, N = compact ? k : n;
    const size_t vs = gb_type_size(uv.tcode);
    if (uv.iso) {
        if (how == HOW_SMALLEST || how == HOW_LARGEST || (how == HOW_RANDOM && compact && !asindex)) {
            how = HOW_FIRST;
            if (compact) reverse = false;
        }
    }
    if (how == HOW_RANDOM) reverse = false;
    const bool wiso = uv.iso && !asindex;
    gb_vec_result T = gb_new_vec_result(N, asindex ? GBAMD_T_UINT64 : uv.tcode, wiso);
    const size_t os = asindex ? sizeof(uint64_t) : vs;
    if (N == 0) {
        gb_memset(T.d_nvals, 0, sizeof(int64_t));
    } else if (n == 0) {
        gb_zero_bitmap(T.bits, gb_words(N), T.d_nvals);
        gb_memset(T.dense, 0, (wiso ? 1 : N) * os);
    } else {
        gb_scratch s;
        const int mode = how == HOW_RANDOM ? 2 : (how == HOW_SMALLEST || how == HOW_LARGEST) ? 1 : 0;
        bool far = how == HOW_LAST || how == HOW_LARGEST;
        int64_t *idx, *off;
        gb_bitmap_order(n, uv.bits, uv.vals, uv.tcode, uv.iso, mode, seed, s, &idx, &off);
        if (wiso) gb_copy_d2d(T.dense, uv.vals, vs);
        const unsigned ngrid = gb_sort_grid(n, SELK_BLOCK);
        if (!compact || how == HOW_RANDOM) {
            uint64_t *keepbits = s.get<uint64_t>(gb_words(n));
            gb_memset(keepbits, 0, gb_words(n) * sizeof(uint64_t));
            hipLaunchKernelGGL(k_selk_vec_mark, dim3(ngrid), dim3(SELK_BLOCK), 0, gb_stream(), n,
                               (const int64_t *)off, (const int64_t *)idx, k, far, (unsigned long long *)keepbits);
            GB_LAUNCH_CHECK();
            if (!compact) {
                hipLaunchKernelGGL(k_selk_vec_select, dim3(ngrid), dim3(SELK_BLOCK), 0, gb_stream(), n,
                                   (const int64_t *)off, k, (const uint64_t *)keepbits, uv.vals, (int)vs,
                                   wiso ? nullptr : T.dense, T.bits, T.d_nvals);
                GB_LAUNCH_CHECK();
            } else {  // the chosen entries, listed again by index
                gb_bitmap_order(n, keepbits, nullptr, 0, false, 0, 0, s, &idx, &off);
                far = false;
            }
        }
        if (compact) {
            hipLaunchKernelGGL(k_selk_vec_emit, dim3(gb_sort_grid(N, SELK_BLOCK)), dim3(SELK_BLOCK), 0, gb_stream(), N,
                               n, (const int64_t *)off, (const int64_t *)idx, far, reverse, uv.vals, (int)vs,
                               asindex || wiso ? nullptr : T.dense, asindex ? (uint64_t *)T.dense : nullptr, T.bits,
                               T.d_nvals);
            GB_LAUNCH_CHECK();
        }
    }
    const gb_desc d0;
    gb_writeback_vector(W, T, nullptr, d0, nullptr, false);
}

}  // namespace

bool gb_selectk_stat(const char *key, int64_t *value) {
    // all: [4]; wave: [0]; block: both workgroup sizes, [1] + [3]; long: [2]
    static const char *names[4] = {"stat_selectk_rows_all", "stat_selectk_rows_wave", "stat_selectk_rows_block",
                                   "stat_selectk_rows_long"};
    static const int slot[4] = {4, 0, 1, 2};
    for (int c = 0; c < 4; c++) {
        if (strcmp(key, names[c])) continue;
        *value = g_selk_stats ? gb_read_i64((const int64_t *)g_selk_stats + slot[c]) : 0;
        if (c == 2 && g_selk_stats) *value += gb_read_i64((const int64_t *)g_selk_stats + 3);
        return true;
    }
    // the class bounds read back as their defaults while unset
    for (const auto &kd :
         {std::make_pair("selectk_wave_max", SELK_WAVE_CAP), std::make_pair("selectk_block_max", SELK_BLOCK_CAP)}) {
        if (strcmp(key, kd.first)) continue;
        *value = selk_knob(kd.first, kd.second);
        return true;
    }
    return false;
}

extern "C" {

GrB_Info GxB_Matrix_selectk(GrB_Matrix C, const GrB_Matrix A, int how, GrB_Index k, uint64_t seed,
                            const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_REQUIRE(C && A, GrB_NULL_POINTER, "C or A is NULL");
        matrix_selectk(gb_obj_check(C), gb_obj_check(A), how, clamp_k(k), false, false, false, seed,
                       gb_read_desc(desc));
    });
}

GrB_Info GxB_Matrix_compactify(GrB_Matrix C, const GrB_Matrix A, int how, GrB_Index k, bool reverse, bool asindex,
                               uint64_t seed, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_REQUIRE(C && A, GrB_NULL_POINTER, "C or A is NULL");
        matrix_selectk(gb_obj_check(C), gb_obj_check(A), how, clamp_k(k), true, reverse, asindex, seed,
                       gb_read_desc(desc));
    });
}

GrB_Info GxB_Vector_selectk(GrB_Vector w, const GrB_Vector u, int how, GrB_Index k, uint64_t seed,
                            const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_REQUIRE(w && u, GrB_NULL_POINTER, "w or u is NULL");
        gb_read_desc(desc);
        vector_selectk(gb_obj_check(w), gb_obj_check(u), how, clamp_k(k), false, false, false, seed);
    });
}

GrB_Info GxB_Vector_compactify(GrB_Vector w, const GrB_Vector u, int how, GrB_Index k, bool reverse, bool asindex,
                               uint64_t seed, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_REQUIRE(w && u, GrB_NULL_POINTER, "w or u is NULL");
        gb_read_desc(desc);
        vector_selectk(gb_obj_check(w), gb_obj_check(u), how, clamp_k(k), true, reverse, asindex, seed);
    });
}

GrB_Info GxB_Matrix_compactify_width(GrB_Index *k, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(nullptr, [&] {
        GB_REQUIRE(k && A, GrB_NULL_POINTER, "k or A is NULL");
        GB_Obj *a = gb_obj_check(A);
        const gb_desc d = gb_read_desc(desc);
        gb_csr_view v;
        if (d.tran0) gb_get_csc(v, a);
        else gb_get_csr(v, a);
        *k = 0;
        if (v.nvals == 0) return;
        gb_scratch s;
        unsigned long long *longest = s.get<unsigned long long>(1);
        gb_memset(longest, 0, sizeof(unsigned long long));
        hipLaunchKernelGGL(k_selk_lens, dim3(gb_sort_grid(v.nrows, SELK_BLOCK)), dim3(SELK_BLOCK), 0, gb_stream(),
                           v.nrows, v.rowptr, (int64_t)0, (int64_t *)nullptr, (unsigned long long *)nullptr, longest);
        GB_LAUNCH_CHECK();
        *k = (GrB_Index)gb_read_i64((const int64_t *)longest);
    });
}

}  // extern "C"
