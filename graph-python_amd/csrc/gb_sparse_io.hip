// gb_sparse_io.hip -- sparse import and export from host or device arrays: COO, CSR and CSC of a
// matrix, indices plus values of a vector (GxB_{Matrix,Vector}_{import,export}_sparse).
//
// The arrays are read and written on the library stream in the caller's own index width (INT32,
// INT64, UINT64) and value type, so an edge list that lives on the device never leaves it.  What
// comes after staging is the build's own device core (gb_coo_fold / gb_build_install in
// gb_object.hip); this file holds the passes around it:
//   k_sio_keys     typed row / column arrays -> row << 32 | col keys and the identity permutation,
//                  with the bounds check and the "already strictly increasing" flag
//   k_sio_ptr      pointer array -> int64 row pointer, with Ap[0] == 0, monotonicity and Ap[last]
//   k_sio_rows     a wave per row: indices -> int32, bounds check, strict order within the row
//   k_sio_convert  int32 / int64 index arrays to the other width (export)
//   k_sio_fill     an iso value written n times (export)
// No kernel uses a caller's pointer or index as an address or a loop bound before it was checked:
// k_sio_ptr reads Ap[0 .. np) only, the host compares its flags and Ap[last] with the lengths it
// was given, and only then does k_sio_rows walk the rows; k_sio_keys uses indices as numbers.
// Every grid comes from gb_sort_grid, the sort's single gb_grid call site.
#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SIO_BLOCK 256
#define SIO_ROWS_CAP 8192  // blocks of gb_rows_of, as gb_object.hip's

namespace {

// ------------------------------------------------------------------ 16-byte accesses
// A lane moves G consecutive elements; when their address is 16-byte aligned that is one
// dwordx4 access per 16 bytes, else one access per element.  A kernel starts its groups after a
// scalar head that aligns the caller's array (a slice such as edge_index[1] starts anywhere) and
// ends with a scalar tail; the other arrays of the same kernel are aligned or not, as it falls.
template <class T, int G>
__device__ inline void sio_ld(const T *__restrict__ p, T (&r)[G]) {
    static_assert((G * sizeof(T)) % 16 == 0, "whole 16-byte pieces");
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        uint4 v[G * sizeof(T) / 16];
#pragma unroll
        for (int k = 0; k < (int)(G * sizeof(T) / 16); k++) v[k] = reinterpret_cast<const uint4 *>(p)[k];
        memcpy(r, v, sizeof(v));
    } else {
#pragma unroll
        for (int e = 0; e < G; e++) r[e] = p[e];
    }
}
template <class T, int G>
__device__ inline void sio_st(T *__restrict__ p, const T (&r)[G]) {
    static_assert((G * sizeof(T)) % 16 == 0, "whole 16-byte pieces");
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        uint4 v[G * sizeof(T) / 16];
        memcpy(v, r, sizeof(v));
#pragma unroll
        for (int k = 0; k < (int)(G * sizeof(T) / 16); k++) reinterpret_cast<uint4 *>(p)[k] = v[k];
    } else {
#pragma unroll
        for (int e = 0; e < G; e++) p[e] = r[e];
    }
}
// elements before p reaches a 16-byte boundary (all n when p is not even aligned for its type)
template <class T>
__device__ inline int64_t sio_head(const T *p, int64_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a % sizeof(T)) return n;
    const int64_t h = (int64_t)(((16 - (a & 15)) & 15) / sizeof(T));
    return h < n ? h : n;
}

// an index as a number: a negative one becomes huge and fails every bound, it never wraps
template <class IT>
__device__ inline uint64_t sio_u64(IT x) {
    return (uint64_t)(int64_t)x;
}

// ------------------------------------------------------------------ keys
template <class IT, class JT>
__device__ inline uint64_t sio_key(uint64_t i, uint64_t j, uint64_t nrows, uint64_t ncols, bool &bad) {
    if (i >= nrows || j >= ncols) {
        bad = true;
        return 0;
    }
    return (i << 32) | j;
}

// keys[q] = I[q] << 32 | J[q] (J null: 0), perm[q] = q; flags[0]: an index out of bounds (its key
// is 0), flags[1]: some key is not greater than its predecessor
template <class IT, class JT>
__global__ __launch_bounds__(SIO_BLOCK) void k_sio_keys(const IT *__restrict__ I, const JT *__restrict__ J, int64_t n,
                                                        uint64_t nrows, uint64_t ncols, uint64_t *__restrict__ keys,
                                                        int64_t *__restrict__ perm, int *__restrict__ flags) {
    constexpr int G = 16 / sizeof(IT);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t h = sio_head(I, n), ngroups = (n - h) / G, tail0 = h + ngroups * G;
    bool bad = false, unsorted = false;
    for (int64_t g = tid; g < ngroups; g += nth) {
        const int64_t q = h + g * G;
        IT iv[G];
        sio_ld<IT, G>(I + q, iv);
        uint64_t jv[G];
        if (J) {
            if constexpr (sizeof(JT) == sizeof(IT)) {
                JT jt[G];
                sio_ld<JT, G>(J + q, jt);
#pragma unroll
                for (int e = 0; e < G; e++) jv[e] = sio_u64(jt[e]);
            } else {
#pragma unroll
                for (int e = 0; e < G; e++) jv[e] = sio_u64(J[q + e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < G; e++) jv[e] = 0;
        }
        bool pbad = false;
        uint64_t prev = q ? sio_key<IT, JT>(sio_u64(I[q - 1]), J ? sio_u64(J[q - 1]) : 0, nrows, ncols, pbad) : 0;
        uint64_t k[G];
        int64_t id[G];
#pragma unroll
        for (int e = 0; e < G; e++) {
            k[e] = sio_key<IT, JT>(sio_u64(iv[e]), jv[e], nrows, ncols, bad);
            if ((q + e) && k[e] <= prev) unsorted = true;
            prev = k[e];
            id[e] = q + e;
        }
        sio_st<uint64_t, G>(keys + q, k);
        sio_st<int64_t, G>(perm + q, id);
    }
    const int64_t nscalar = h + (n - tail0);  // the head and the tail
    for (int64_t t = tid; t < nscalar; t += nth) {
        const int64_t q = t < h ? t : tail0 + (t - h);
        const uint64_t k = sio_key<IT, JT>(sio_u64(I[q]), J ? sio_u64(J[q]) : 0, nrows, ncols, bad);
        if (q) {
            bool pbad = false;
            if (k <= sio_key<IT, JT>(sio_u64(I[q - 1]), J ? sio_u64(J[q - 1]) : 0, nrows, ncols, pbad)) unsorted = true;
        }
        keys[q] = k;
        perm[q] = q;
    }
    if (bad) flags[0] = 1;
    if (unsorted) flags[1] = 1;
}

// ------------------------------------------------------------------ compressed input
// rp[q] = Ap[q] for q < np; out[0] bit 0: Ap[0] != 0, bit 1: Ap decreases somewhere; out[1] = Ap[np - 1].
// A pointer that starts at 0, never decreases and ends at most at Ai_len (the host's comparison)
// has every value inside [0, Ai_len]: a negative one is huge here and breaks one of the three.
template <class IT>
__global__ __launch_bounds__(SIO_BLOCK) void k_sio_ptr(const IT *__restrict__ Ap, int64_t np, int64_t *__restrict__ rp,
                                                       unsigned long long *__restrict__ out) {
    unsigned f = 0;
    GB_GRID_LOOP(q, np) {
        const uint64_t x = sio_u64(Ap[q]);
        rp[q] = (int64_t)x;
        if (q == 0 && x != 0) f |= 1;
        if (q > 0 && x < sio_u64(Ap[q - 1])) f |= 2;
        if (q == np - 1) out[1] = x;
    }
    if (f) atomicOr(&out[0], (unsigned long long)f);
}

// a wave per row of a checked pointer: ci[p] = Ai[p] as int32; flags[0]: an index >= ncols (or
// negative), flags[1]: a row that is not strictly increasing.  Touches Ai[0 .. rp[nrows]) only.
template <class IT>
__global__ __launch_bounds__(SIO_BLOCK) void k_sio_rows(const int64_t *__restrict__ rp, int64_t nrows,
                                                        const IT *__restrict__ Ai, uint64_t ncols,
                                                        int32_t *__restrict__ ci, int *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    bool bad = false, jumbled = false;
    for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; r < nrows; r += nwaves) {
        const int64_t lo = rp[r], hi = rp[r + 1];
        for (int64_t p = lo + lane; p < hi; p += 64) {
            uint64_t x = sio_u64(Ai[p]);
            if (p > lo && x <= sio_u64(Ai[p - 1])) jumbled = true;
            if (x >= ncols) {
                bad = true;
                x = 0;
            }
            ci[p] = (int32_t)x;
        }
    }
    if (bad) flags[0] = 1;
    if (jumbled) flags[1] = 1;
}

// ------------------------------------------------------------------ export
// dst[q] = src[q] in the other width: 4 elements per lane, the head aligns dst (the caller's)
template <class S, class D>
__global__ __launch_bounds__(SIO_BLOCK) void k_sio_convert(const S *__restrict__ src, D *__restrict__ dst, int64_t n) {
    constexpr int G = 4;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t h = sio_head(dst, n), ngroups = (n - h) / G, tail0 = h + ngroups * G;
    for (int64_t g = tid; g < ngroups; g += nth) {
        const int64_t q = h + g * G;
        S a[G];
        D b[G];
        sio_ld<S, G>(src + q, a);
#pragma unroll
        for (int e = 0; e < G; e++) b[e] = (D)a[e];
        sio_st<D, G>(dst + q, b);
    }
    const int64_t nscalar = h + (n - tail0);
    for (int64_t t = tid; t < nscalar; t += nth) {
        const int64_t q = t < h ? t : tail0 + (t - h);
        dst[q] = (D)src[q];
    }
}

// dst[q] = *one for q < n, 16 bytes per lane
template <class W>
__global__ __launch_bounds__(SIO_BLOCK) void k_sio_fill(W *__restrict__ dst, const W *__restrict__ one, int64_t n) {
    constexpr int G = 16 / sizeof(W);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t h = sio_head(dst, n), ngroups = (n - h) / G, tail0 = h + ngroups * G;
    const W x = *one;
    W b[G];
#pragma unroll
    for (int e = 0; e < G; e++) b[e] = x;
    for (int64_t g = tid; g < ngroups; g += nth) sio_st<W, G>(dst + h + g * G, b);
    const int64_t nscalar = h + (n - tail0);
    for (int64_t t = tid; t < nscalar; t += nth) dst[t < h ? t : tail0 + (t - h)] = x;
}

// ------------------------------------------------------------------ host side
unsigned lane_grid(int64_t lanes) { return gb_sort_grid(lanes, SIO_BLOCK); }
unsigned wave_grid(int64_t waves) { return gb_sort_grid(waves, SIO_BLOCK / 64); }

// INT32 / INT64 / UINT64 -> bytes per index
int index_size(GrB_Type t) {
    GB_REQUIRE(t && t->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid index type");
    GB_REQUIRE(t->code == GBAMD_T_INT32 || t->code == GBAMD_T_INT64 || t->code == GBAMD_T_UINT64, GrB_DOMAIN_MISMATCH,
               "index_type must be GrB_INT32, GrB_INT64 or GrB_UINT64");
    return t->code == GBAMD_T_INT32 ? 4 : 8;
}
template <class F>
void with_index(int icode, F &&f) {
    if (icode == GBAMD_T_INT32) f(int32_t());
    else if (icode == GBAMD_T_INT64) f(int64_t());
    else f(uint64_t());
}

// a host array's device copy (one copy), or the device array itself
const void *stage_in(const void *p, size_t bytes, bool on_device, gb_scratch &s) {
    if (on_device || !p || !bytes) return p;
    char *d = s.get<char>(bytes);
    gb_copy_h2d(d, p, bytes);
    return d;
}

// the n values at X (device, xcode) as type `code`: X itself, or a cast copy in s
const void *values_as(const void *X, int xcode, int code, int64_t n, gb_scratch &s) {
    if (xcode == code) return X;
    void *c = s.get<char>(n * gb_type_size(code));
    gb_cast_array(c, code, X, xcode, n);
    return c;
}

template <class IT, class JT>
void launch_keys(const void *I, const void *J, int64_t n, int64_t nrows, int64_t ncols, uint64_t *keys, int64_t *perm,
                 int *flags) {
    hipLaunchKernelGGL((k_sio_keys<IT, JT>), dim3(lane_grid(n / (16 / sizeof(IT)) + 8)), dim3(SIO_BLOCK), 0,
                       gb_stream(), (const IT *)I, (const JT *)J, n, (uint64_t)nrows, (uint64_t)ncols, keys, perm,
                       flags);
    GB_LAUNCH_CHECK();
}

// C (empty, its shape set) = the n tuples I, J (J null: a vector), X: device arrays.  icode: the
// index type; X holds n values, or one when x_iso, in xcode.
void import_coo(GB_Obj *C, const void *I, const void *J, const void *X, int icode, int xcode, int64_t n, bool x_iso,
                GrB_BinaryOp dup) {
    gb_stat_set("sparse_import_path", 0);
    if (n == 0) return;
    const bool is_vec = C->kind != GB_KIND_MATRIX;
    const int64_t nrows = C->nrows, ncols = is_vec ? 1 : C->ncols;
    GB_REQUIRE(nrows < (1LL << 31), GrB_OUT_OF_MEMORY, "2^31 or more rows exceed the build's key width");
    const int code = C->type->code;
    const size_t ts = C->type->size;
    gb_scratch s;
    uint64_t *keys = gb_malloc_n<uint64_t>(n);  // the direct path hands them to the install
    void *uvals = nullptr;                       // the direct path's values, until the install has them
    try {
        int64_t *perm = s.get<int64_t>(n);
        int *flags = s.get<int>(2);
        gb_memset(flags, 0, 2 * sizeof(int));
        with_index(icode, [&](auto z) {
            using IT = decltype(z);
            launch_keys<IT, IT>(I, is_vec ? nullptr : J, n, nrows, ncols, keys, perm, flags);
        });
        int h[2];
        gb_copy_d2h(h, flags, sizeof(h));
        GB_REQUIRE(!h[0], GrB_INDEX_OUT_OF_BOUNDS, "index out of bounds in import");
        const int64_t nx = x_iso ? 1 : n;
        if (!h[1]) {  // strictly increasing: nothing to sort or fold
            const void *Xc = x_iso ? values_as(X, xcode, code, 1, s) : nullptr;
            if (!x_iso) {
                uvals = gb_malloc(n * ts);
                gb_cast_array(uvals, code, X, xcode, n);
            } else if (!gb_build_keeps_iso(dup)) {
                uvals = gb_expand_iso(Xc, ts, n);
            }
            uint64_t *uk = keys;
            void *uv = uvals;
            keys = nullptr;  // the install owns both from here on
            uvals = nullptr;
            gb_build_install(C, uk, uv, n, Xc, x_iso, dup);
            return;
        }
        gb_stat_set("sparse_import_path", 1);
        const void *Xc = values_as(X, xcode, code, nx, s);
        uint64_t *ukeys;
        void *fvals;
        int64_t nu;
        gb_coo_fold(keys, perm, Xc, x_iso, n, nrows, code, dup ? dup->opcode : -1, &ukeys, &fvals, &nu);
        gb_free(keys);
        keys = nullptr;
        gb_build_install(C, ukeys, fvals, nu, Xc, x_iso, dup);
    } catch (...) {
        gb_free(keys);
        gb_free(uvals);
        throw;
    }
}

// C (empty, pr x pc) = the CSR Ap, Ai, Ax (host or device arrays)
void import_csx(GB_Obj *C, const void *Ap, const void *Ai, const void *Ax, int icode, int isz, int xcode,
                uint64_t Ap_len, uint64_t Ai_len, uint64_t Ax_len, bool on_device) {
    const int64_t pr = C->nrows, pc = C->ncols, np = pr + 1;
    const int code = C->type->code;
    const size_t ts = C->type->size, xs = gb_type_size(xcode);
    gb_stat_set("sparse_import_path", 0);
    GB_REQUIRE(Ap_len >= (uint64_t)np, GrB_INVALID_VALUE, "Ap is shorter than the dimension + 1");
    GB_REQUIRE(Ap, GrB_NULL_POINTER, "Ap is NULL");
    GB_REQUIRE(pr < (1LL << 31), GrB_OUT_OF_MEMORY, "2^31 or more rows exceed the build's key width");
    gb_scratch s;
    int64_t *rp = gb_malloc_n<int64_t>(np);
    int32_t *ci = nullptr;
    void *vx = nullptr;
    try {
        // the pointer check, before anything is addressed through the pointer
        const void *dAp = stage_in(Ap, np * isz, on_device, s);
        unsigned long long *out = s.get<unsigned long long>(2);
        gb_memset(out, 0, 2 * sizeof(unsigned long long));
        with_index(icode, [&](auto z) {
            using IT = decltype(z);
            hipLaunchKernelGGL((k_sio_ptr<IT>), dim3(lane_grid(np)), dim3(SIO_BLOCK), 0, gb_stream(), (const IT *)dAp,
                               np, rp, out);
        });
        GB_LAUNCH_CHECK();
        unsigned long long h[2];
        gb_copy_d2h(h, out, sizeof(h));
        const uint64_t last = h[1];
        GB_REQUIRE(h[0] == 0, GrB_INVALID_VALUE, "Ap must start at 0 and never decrease");
        GB_REQUIRE(last <= Ai_len, GrB_INVALID_VALUE, "Ap ends past the index array");
        GB_REQUIRE(Ax_len == 1 || Ax_len >= last, GrB_INVALID_VALUE, "Ax holds neither one value nor one per entry");
        const int64_t nz = (int64_t)last;
        if (nz == 0) {
            gb_install_csr(C, pr, pc, 0, rp, nullptr, nullptr, false);
            return;
        }
        GB_REQUIRE(Ai && Ax, GrB_NULL_POINTER, "NULL import array");
        const void *dAi = stage_in(Ai, nz * isz, on_device, s);
        ci = gb_malloc_n<int32_t>(nz);
        int *flags = s.get<int>(2);
        gb_memset(flags, 0, 2 * sizeof(int));
        with_index(icode, [&](auto z) {
            using IT = decltype(z);
            hipLaunchKernelGGL((k_sio_rows<IT>), dim3(wave_grid(pr)), dim3(SIO_BLOCK), 0, gb_stream(), rp, pr,
                               (const IT *)dAi, (uint64_t)pc, ci, flags);
        });
        GB_LAUNCH_CHECK();
        int f[2];
        gb_copy_d2h(f, flags, sizeof(f));
        GB_REQUIRE(!f[0], GrB_INDEX_OUT_OF_BOUNDS, "index out of bounds in import");
        const bool x_iso = Ax_len == 1 && nz > 1;
        const int64_t nx = x_iso ? 1 : nz;
        const void *dAx = stage_in(Ax, nx * xs, on_device, s);
        if (!f[1]) {  // sorted rows without duplicates: installed as they are
            vx = gb_malloc(nx * ts);
            gb_cast_array(vx, code, dAx, xcode, nx);
            if (!on_device) gb_sync();  // the host arrays have been read
            gb_install_csr(C, pr, pc, nz, rp, ci, vx, x_iso);
            return;
        }
        // a jumbled row or a duplicate: row-of expansion, then the COO core (the last one is kept)
        gb_stat_set("sparse_import_path", 2);
        int64_t *rows = s.get<int64_t>(nz);
        gb_rows_of(rp, 0, pr, 0, rows, SIO_ROWS_CAP);
        uint64_t *keys = s.get<uint64_t>(nz);
        int64_t *perm = s.get<int64_t>(nz);
        launch_keys<int64_t, int32_t>(rows, ci, nz, pr, pc, keys, perm, flags);
        const void *Xc = values_as(dAx, xcode, code, nx, s);
        uint64_t *ukeys;
        void *uvals;
        int64_t nu;
        gb_coo_fold(keys, perm, Xc, x_iso, nz, pr, code, -1, &ukeys, &uvals, &nu);
        gb_free(rp);
        gb_free(ci);
        rp = nullptr;
        ci = nullptr;
        gb_build_install(C, ukeys, uvals, nu, Xc, x_iso, nullptr);
    } catch (...) {
        gb_free(rp);
        gb_free(ci);
        gb_free(vx);
        throw;
    }
}

void free_object(GB_Obj *o) {
    GrB_Matrix m = (GrB_Matrix)o;
    GrB_Matrix_free(&m);
}

// n indices from a device array of ssz-byte elements to dst in isz bytes each
void put_indices(void *dst, int isz, bool on_device, const void *src, int ssz, int64_t n, gb_scratch &s) {
    if (n == 0 || !dst || dst == src) return;
    if (ssz == isz) {
        if (on_device) gb_copy_d2d(dst, src, n * isz);
        else gb_copy_d2h(dst, src, n * isz);
        return;
    }
    void *d = on_device ? dst : s.get<char>(n * isz);
    if (ssz == 4)
        hipLaunchKernelGGL((k_sio_convert<int32_t, int64_t>), dim3(lane_grid(n / 4 + 8)), dim3(SIO_BLOCK), 0,
                           gb_stream(), (const int32_t *)src, (int64_t *)d, n);
    else
        hipLaunchKernelGGL((k_sio_convert<int64_t, int32_t>), dim3(lane_grid(n / 4 + 8)), dim3(SIO_BLOCK), 0,
                           gb_stream(), (const int64_t *)src, (int32_t *)d, n);
    GB_LAUNCH_CHECK();
    if (!on_device) gb_copy_d2h(dst, d, n * isz);
}

// n values of type vcode to dst from the device array src (scode; one value when iso)
void put_values(void *dst, int vcode, bool on_device, const void *src, int scode, bool iso, int64_t n, gb_scratch &s) {
    if (n == 0 || !dst) return;
    const size_t vs = gb_type_size(vcode);
    if (!on_device && !iso && vcode == scode) {
        gb_copy_d2h(dst, src, n * vs);
        return;
    }
    void *d = on_device ? dst : s.get<char>(n * vs);
    if (iso) {
        const void *one = values_as(src, scode, vcode, 1, s);
        gb_with_size(vs, [&](auto w) {
            using W = decltype(w);
            hipLaunchKernelGGL((k_sio_fill<W>), dim3(lane_grid(n * sizeof(W) / 16 + 8)), dim3(SIO_BLOCK), 0, gb_stream(),
                               (W *)d, (const W *)one, n);
        });
        GB_LAUNCH_CHECK();
    } else if (d != src) {
        gb_cast_array(d, vcode, src, scode, n);  // the same type: one copy
    }
    if (!on_device) gb_copy_d2h(dst, d, n * vs);
}

// INT32 indices hold a dimension or a count below 2^31 only
void check_width(int isz, int64_t a, int64_t b, int64_t c) {
    GB_REQUIRE(isz == 8 || (a < (1LL << 31) && b < (1LL << 31) && c < (1LL << 31)), GrB_INVALID_VALUE,
               "a dimension or nvals does not fit a GrB_INT32 index");
}

void export_matrix_sparse(void *Ap, void *Ai, void *Ax, int isz, int vcode, GrB_Index *Ap_len, GrB_Index *Ai_len,
                          GrB_Index *Ax_len, GrB_Format format, GB_Obj *A, bool on_device) {
    GB_REQUIRE(A->kind == GB_KIND_MATRIX, GrB_INVALID_OBJECT, "not a matrix");
    GB_REQUIRE(format == GrB_CSR_FORMAT || format == GrB_CSC_FORMAT || format == GrB_COO_FORMAT, GrB_INVALID_VALUE,
               "unknown format");
    const int64_t nz = A->nvals;
    check_width(isz, A->nrows, A->ncols, nz);
    const int64_t np = format == GrB_COO_FORMAT ? nz : (format == GrB_CSR_FORMAT ? A->nrows : A->ncols) + 1;
    GB_REQUIRE((!Ap || (int64_t)*Ap_len >= np) && (!Ai || (int64_t)*Ai_len >= nz) && (!Ax || (int64_t)*Ax_len >= nz),
               GrB_INSUFFICIENT_SPACE, "export arrays too small");
    gb_csr_view v;
    if (format == GrB_CSC_FORMAT) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    gb_scratch s;
    if (Ap && format == GrB_COO_FORMAT && nz) {
        int64_t *rows = (on_device && isz == 8) ? (int64_t *)Ap : s.get<int64_t>(nz);
        gb_rows_of(v.rowptr, 0, v.nrows, 0, rows, SIO_ROWS_CAP);
        put_indices(Ap, isz, on_device, rows, 8, nz, s);
    } else if (Ap) {
        put_indices(Ap, isz, on_device, v.rowptr, 8, np, s);
    }
    if (Ai) put_indices(Ai, isz, on_device, v.colidx, 4, nz, s);
    if (Ax) put_values(Ax, vcode, on_device, v.vals, v.tcode, v.iso, nz, s);
    *Ap_len = np;
    *Ai_len = nz;
    *Ax_len = Ax ? nz : 0;
}

void export_vector_sparse(void *Ai, void *Ax, int isz, int vcode, GrB_Index *Ai_len, GrB_Index *Ax_len, GB_Obj *v,
                          bool on_device) {
    GB_REQUIRE(v->kind != GB_KIND_MATRIX, GrB_INVALID_OBJECT, "not a vector");
    const int64_t nz = gb_nvals(v);
    check_width(isz, v->nrows, 0, nz);
    GB_REQUIRE((!Ai || (int64_t)*Ai_len >= nz) && (!Ax || (int64_t)*Ax_len >= nz), GrB_INSUFFICIENT_SPACE,
               "export arrays too small");
    if (nz) {
        gb_scratch s;
        const int scode = v->type->code;
        uint64_t *dI = (Ai && on_device && isz == 8) ? (uint64_t *)Ai : s.get<uint64_t>(nz);
        const bool want_vals = Ax && !v->iso;
        void *dX = !want_vals ? nullptr : (on_device && vcode == scode) ? Ax : s.get<char>(nz * v->type->size);
        gb_vector_tuples(v, dI, dX);
        if (Ai) put_indices(Ai, isz, on_device, dI, 8, nz, s);
        if (Ax) put_values(Ax, vcode, on_device, v->iso ? v->dense : dX, scode, v->iso, nz, s);
    }
    *Ai_len = nz;
    *Ax_len = Ax ? nz : 0;
}

}  // namespace

extern "C" {

GrB_Info GxB_Matrix_import_sparse(GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void *Ap,
                                  const void *Ai, const void *Ax, GrB_Type index_type, GrB_Type value_type,
                                  GrB_Index Ap_len, GrB_Index Ai_len, GrB_Index Ax_len, GrB_Format format,
                                  const GrB_BinaryOp dup, bool on_device) {
    if (!A) return GrB_NULL_POINTER;
    return gb_api(nullptr, [&] {
        const int isz = index_size(index_type);
        GB_REQUIRE(value_type && value_type->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid value type");
        gb_check_binop(dup, true);
        const int icode = index_type->code, xcode = value_type->code;
        if (format == GrB_COO_FORMAT) {
            GB_REQUIRE(Ap_len == Ai_len && (Ax_len == 1 || Ax_len >= Ai_len), GrB_INVALID_VALUE, "bad COO lengths");
            GB_REQUIRE(Ai_len == 0 || (Ap && Ai && Ax), GrB_NULL_POINTER, "NULL import array");
            GB_Obj *o = gb_new_object(GB_KIND_MATRIX, type, nrows, ncols);
            try {
                const int64_t n = (int64_t)Ai_len;
                const bool x_iso = Ax_len == 1 && n > 1;
                gb_scratch s;
                const void *dI = stage_in(Ap, n * isz, on_device, s);
                const void *dJ = stage_in(Ai, n * isz, on_device, s);
                const void *dX = stage_in(Ax, (x_iso ? 1 : n) * gb_type_size(xcode), on_device, s);
                import_coo(o, dI, dJ, dX, icode, xcode, n, x_iso, dup);
                if (!on_device) gb_sync();  // the host arrays have been read
            } catch (...) {
                free_object(o);
                throw;
            }
            *A = (GrB_Matrix)o;
            return;
        }
        GB_REQUIRE(format == GrB_CSR_FORMAT || format == GrB_CSC_FORMAT, GrB_INVALID_VALUE, "unknown format");
        const bool csc = format == GrB_CSC_FORMAT;
        GB_Obj *o = gb_new_object(GB_KIND_MATRIX, type, nrows, ncols);
        GB_Obj *t = nullptr;
        try {
            if (!csc) {
                import_csx(o, Ap, Ai, Ax, icode, isz, xcode, Ap_len, Ai_len, Ax_len, on_device);
            } else {  // the CSR of the transpose, transposed on the device
                t = gb_new_object(GB_KIND_MATRIX, type, ncols, nrows);
                import_csx(t, Ap, Ai, Ax, icode, isz, xcode, Ap_len, Ai_len, Ax_len, on_device);
                if (t->nvals) {
                    int64_t *rp;
                    int32_t *ci;
                    void *vx;
                    gb_transpose_csr(t->nrows, t->ncols, t->nvals, t->rowptr, t->colidx, t->vals, type->size, t->iso,
                                     &rp, &ci, &vx);
                    gb_install_csr(o, (int64_t)nrows, (int64_t)ncols, t->nvals, rp, ci, vx, t->iso);
                }
                free_object(t);
                t = nullptr;
            }
        } catch (...) {
            if (t) free_object(t);
            free_object(o);
            throw;
        }
        *A = (GrB_Matrix)o;
    });
}

GrB_Info GxB_Vector_import_sparse(GrB_Vector *v, GrB_Type type, GrB_Index n, const void *Ai, const void *Ax,
                                  GrB_Type index_type, GrB_Type value_type, GrB_Index Ai_len, GrB_Index Ax_len,
                                  const GrB_BinaryOp dup, bool on_device) {
    if (!v) return GrB_NULL_POINTER;
    return gb_api(nullptr, [&] {
        const int isz = index_size(index_type);
        GB_REQUIRE(value_type && value_type->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid value type");
        gb_check_binop(dup, true);
        GB_REQUIRE(Ax_len == 1 || Ax_len >= Ai_len, GrB_INVALID_VALUE, "bad lengths");
        GB_REQUIRE(Ai_len == 0 || (Ai && Ax), GrB_NULL_POINTER, "NULL import array");
        GB_Obj *o = gb_new_object(GB_KIND_VECTOR, type, n, 1);
        try {
            const int64_t m = (int64_t)Ai_len;
            const bool x_iso = Ax_len == 1 && m > 1;
            gb_scratch s;
            const void *dI = stage_in(Ai, m * isz, on_device, s);
            const void *dX = stage_in(Ax, (x_iso ? 1 : m) * gb_type_size(value_type->code), on_device, s);
            import_coo(o, dI, nullptr, dX, index_type->code, value_type->code, m, x_iso, dup);
            if (!on_device) gb_sync();
        } catch (...) {
            free_object(o);
            throw;
        }
        *v = (GrB_Vector)o;
    });
}

GrB_Info GxB_Matrix_export_sparse(void *Ap, void *Ai, void *Ax, GrB_Type index_type, GrB_Type value_type,
                                  GrB_Index *Ap_len, GrB_Index *Ai_len, GrB_Index *Ax_len, GrB_Format format,
                                  const GrB_Matrix A, bool on_device) {
    if (!Ap_len || !Ai_len || !Ax_len) return GrB_NULL_POINTER;
    return gb_api(OBJ(A), [&] {
        GB_Obj *o = gb_obj_check(A);
        const int isz = index_size(index_type);
        GB_REQUIRE(value_type && value_type->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid value type");
        export_matrix_sparse(Ap, Ai, Ax, isz, value_type->code, Ap_len, Ai_len, Ax_len, format, o, on_device);
    });
}

GrB_Info GxB_Vector_export_sparse(void *Ai, void *Ax, GrB_Type index_type, GrB_Type value_type, GrB_Index *Ai_len,
                                  GrB_Index *Ax_len, const GrB_Vector v, bool on_device) {
    if (!Ai_len || !Ax_len) return GrB_NULL_POINTER;
    return gb_api(OBJ(v), [&] {
        GB_Obj *o = gb_obj_check(v);
        const int isz = index_size(index_type);
        GB_REQUIRE(value_type && value_type->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid value type");
        export_vector_sparse(Ai, Ax, isz, value_type->code, Ai_len, Ax_len, o, on_device);
    });
}

}  // extern "C"
