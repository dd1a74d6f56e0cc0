// gb_ops.hip -- the general GraphBLAS operations exported by the C ABI:
//   GrB_mxm, eWiseMult / eWiseAdd, assign, apply, reduce, transpose  (loop companions
//   used by python-graphblas's isequal (reference core/matrix.py:391-398) and the
//   BFS/SSSP notebook loops)
// Each call: validate -> views of the inputs (casting values to the operator's
// input type) -> compute T on the device -> C<M,replace> = C accum T.
// GrB_mxv / GrB_vxm and the work the level-BFS loop defers around them (the stamp a scalar
// assign may become, the speculated level) are in gb_bfs_loop.hip, which calls back the
// scalar assigns defined here (gb_vector_assign_scalar, gb_assign_all_scalar_fast).
#include <algorithm>
#include <vector>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define OPS_BLOCK 256
#define OPS_GRID_CAP 16384  // blocks, unless the launch names its own cap

// ================================================================== mxm
static void do_mxm(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *B,
                   const gb_desc &d) {
    gb_check_semiring(sr);
    gb_check_binop(accum, true);
    int64_t ar = d.tran0 ? gb_ncols_of(A) : A->nrows, ac = d.tran0 ? A->nrows : gb_ncols_of(A);
    int64_t br = d.tran1 ? gb_ncols_of(B) : B->nrows, bc = d.tran1 ? B->nrows : gb_ncols_of(B);
    GB_REQUIRE(ac == br, GrB_DIMENSION_MISMATCH, "inner dimensions of A and B do not match");
    GB_REQUIRE(C->nrows == ar && gb_ncols_of(C) == bc, GrB_DIMENSION_MISMATCH, "C dimensions do not match A*B");
    gb_csr_view av, bv, btv;
    if (d.tran0) gb_get_csc(av, A);
    else gb_get_csr(av, A);
    if (d.tran1) gb_get_csc(bv, B);
    else gb_get_csr(bv, B);
    gb_mmask m;
    gb_make_mmask(m, M, d, ar, bc);
    gb_csr_view *btp = nullptr;
    int64_t method = gb_knob("mxm_method");  // 0 auto, 1 dot, 2 gustavson
    if (m.present && !m.comp && method != 2) {
        // B'^T: rows are the columns of B'
        if (d.tran1) gb_get_csr(btv, B);
        else gb_get_csc(btv, B);
        btp = &btv;
        // the masked dot reads one value per matching key: narrow copies of integer values
        if (gb_sr_describe(sr).reads_values) {
            gb_view_narrow(av, A, d.tran0 ? 1 : 0);
            gb_view_narrow(btv, B, d.tran1 ? 0 : 1);
        }
    }
    gb_mat_result T;
    gb_spgemm(T, av, bv, btp, m, sr);
    gb_writeback_matrix(C, T, M, d, accum);
}

// ================================================================== eWise
template <class X, class Z>
__global__ void k_ewise_vec(int64_t n, int op, bool add, const uint64_t *__restrict__ ub, const X *__restrict__ ux,
                            bool u_iso, const uint64_t *__restrict__ vb, const X *__restrict__ vx, bool v_iso,
                            uint64_t *__restrict__ ob, Z *__restrict__ oz, unsigned long long *__restrict__ cnt,
                            unsigned long long *__restrict__ gst) {
    unsigned long long mine = 0;
    for (int64_t base = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~63LL; base < n;
         base += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = base + (threadIdx.x & 63);
        bool a = i < n && gb_bit(ub, i), b = i < n && gb_bit(vb, i);
        bool have = add ? (a || b) : (a && b);
        if (have) {
            if (a && b) oz[i] = gb_binop_z<X, Z>(op, ux[u_iso ? 0 : i], vx[v_iso ? 0 : i], i, 0, 0);
            else if (a) oz[i] = gb_cast<Z, X>(ux[u_iso ? 0 : i]);
            else oz[i] = gb_cast<Z, X>(vx[v_iso ? 0 : i]);
        }
        unsigned long long w = __ballot(have);
        if ((threadIdx.x & 63) == 0) {
            ob[base >> 6] = w;
            mine += __popcll(w);
        }
    }
    gb_grid_add((long long)mine, cnt, gst);
}

template <class X, class Z, bool FILL>
__global__ void k_ewise_mat(int64_t nrows, int op, bool add, const int64_t *__restrict__ arp,
                            const int32_t *__restrict__ aci, const X *__restrict__ ax, bool a_iso,
                            const int64_t *__restrict__ brp, const int32_t *__restrict__ bci, const X *__restrict__ bx,
                            bool b_iso, int64_t *__restrict__ orp, int32_t *__restrict__ oci, Z *__restrict__ oz) {
    GB_GRID_LOOP(i, nrows) {
        int64_t pa = arp[i], ea = arp[i + 1], pb = brp[i], eb = brp[i + 1];
        int64_t o = FILL ? orp[i] : 0;
        while (pa < ea || pb < eb) {
            int32_t ja = pa < ea ? aci[pa] : INT32_MAX, jb = pb < eb ? bci[pb] : INT32_MAX;
            int32_t j = ja < jb ? ja : jb;
            bool a = ja == j, b = jb == j;
            bool have = add ? true : (a && b);
            if (have) {
                if (FILL) {
                    oci[o] = j;
                    if (a && b) oz[o] = gb_binop_z<X, Z>(op, ax[a_iso ? 0 : pa], bx[b_iso ? 0 : pb], i, j, j);
                    else if (a) oz[o] = gb_cast<Z, X>(ax[a_iso ? 0 : pa]);
                    else oz[o] = gb_cast<Z, X>(bx[b_iso ? 0 : pb]);
                }
                o++;
            }
            if (a) pa++;
            if (b) pb++;
        }
        if (!FILL) orp[i] = o;
    }
}

static void do_ewise(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp op, GB_Obj *A, GB_Obj *B,
                     const gb_desc &d, bool add) {
    gb_check_binop(op, false);
    gb_check_binop(accum, true);
    GB_REQUIRE(op->xtype != nullptr, GrB_NOT_IMPLEMENTED, "positional eWise operator");
    int xcode = op->xtype->code, zcode = op->ztype->code;
    bool vec = C->kind != GB_KIND_MATRIX;
    if (vec) {
        int64_t n = C->nrows;
        GB_REQUIRE(A->nrows == n && B->nrows == n && gb_ncols_of(A) == 1 && gb_ncols_of(B) == 1, GrB_DIMENSION_MISMATCH,
                   "vector sizes do not match");
        gb_bitmap_view ua, ub;
        gb_get_bitmap(ua, A);
        gb_get_bitmap(ub, B);
        gb_scratch s;
        const void *xa = gb_bitmap_vals_as(ua, xcode, s), *xb = gb_bitmap_vals_as(ub, xcode, s);
        gb_vec_result T = gb_new_vec_result(n, zcode, false);
        gb_memset(T.d_nvals, 0, sizeof(int64_t));
        gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
            using X = decltype(x);
            using Z = decltype(z);
            if (n)
                hipLaunchKernelGGL((k_ewise_vec<X, Z>), dim3(gb_grid(n, OPS_BLOCK, 1024)), dim3(OPS_BLOCK), 0,
                                   gb_stream(), n, op->opcode, add, ua.bits, (const X *)xa, ua.iso, ub.bits,
                                   (const X *)xb, ub.iso, T.bits, (Z *)T.dense, (unsigned long long *)T.d_nvals,
                                   gb_device_state());
        });
        GB_LAUNCH_CHECK();
        gb_writeback_vector(C, T, M, d, accum, false);
        return;
    }
    int64_t nr = C->nrows, nc = C->ncols;
    GB_Obj *A2 = A, *B2 = B;
    gb_csr_view av, bv;
    if (d.tran0) gb_get_csc(av, A2);
    else gb_get_csr(av, A2);
    if (d.tran1) gb_get_csc(bv, B2);
    else gb_get_csr(bv, B2);
    GB_REQUIRE(av.nrows == nr && av.ncols == nc && bv.nrows == nr && bv.ncols == nc, GrB_DIMENSION_MISMATCH,
               "matrix dimensions do not match");
    gb_scratch s;
    const void *xa = gb_view_vals_as(av, xcode, s), *xb = gb_view_vals_as(bv, xcode, s);
    gb_mat_result T;
    T.nrows = nr;
    T.ncols = nc;
    T.tcode = zcode;
    int64_t *cnt = s.get<int64_t>(nr + 1);
    T.rowptr = gb_malloc_n<int64_t>(nr + 1);
    gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
        using X = decltype(x);
        using Z = decltype(z);
        if (nr)
            hipLaunchKernelGGL((k_ewise_mat<X, Z, false>), dim3(gb_grid(nr, OPS_BLOCK, OPS_GRID_CAP)), dim3(OPS_BLOCK),
                               0, gb_stream(), nr, op->opcode, add, av.rowptr, av.colidx, (const X *)xa, av.iso,
                               bv.rowptr, bv.colidx, (const X *)xb, bv.iso, cnt, nullptr, nullptr);
        GB_LAUNCH_CHECK();
        gb_exclusive_scan_i64(cnt, T.rowptr, nr);
        T.nvals = gb_read_i64(T.rowptr + nr);
        T.colidx = gb_malloc_n<int32_t>(T.nvals);
        T.vals = gb_malloc(T.nvals * sizeof(Z));
        if (nr)
            hipLaunchKernelGGL((k_ewise_mat<X, Z, true>), dim3(gb_grid(nr, OPS_BLOCK, OPS_GRID_CAP)), dim3(OPS_BLOCK),
                               0, gb_stream(), nr, op->opcode, add, av.rowptr, av.colidx, (const X *)xa, av.iso,
                               bv.rowptr, bv.colidx, (const X *)xb, bv.iso, T.rowptr, T.colidx, (Z *)T.vals);
        GB_LAUNCH_CHECK();
    });
    gb_writeback_matrix(C, T, M, d, accum);
}

// ================================================================== reduce
template <class T>
__global__ void k_reduce_partial(int mon, const T *__restrict__ vals, bool iso, int64_t nvals,
                                 const uint64_t *__restrict__ bits, int64_t n, T *__restrict__ part,
                                 int *__restrict__ pfound) {
    // bits == nullptr: reduce vals[0..nvals); else reduce vals[i] for set bits i < n
    __shared__ T sv[256];
    __shared__ int sf[256];
    T acc = T();
    bool found = false;
    int64_t total = bits ? n : nvals;
    GB_GRID_LOOP(i, total) {
        if (bits && !gb_bit(bits, i)) continue;
        T v = vals[iso ? 0 : i];
        acc = found ? gb_monoid<T>(mon, acc, v) : v;
        found = true;
    }
    sv[threadIdx.x] = acc;
    sf[threadIdx.x] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        T a = T();
        bool f = false;
        for (int t = 0; t < blockDim.x; t++)
            if (sf[t]) {
                a = f ? gb_monoid<T>(mon, a, sv[t]) : sv[t];
                f = true;
            }
        part[blockIdx.x] = a;
        pfound[blockIdx.x] = f;
    }
}

// returns true if any entry; value in *out (monoid type)
static bool reduce_values(GB_Obj *A, GrB_Monoid monoid, void *out) {
    GB_REQUIRE(monoid && monoid->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid monoid");
    int code = monoid->type->code;
    gb_scratch s;
    const void *vals;
    bool iso;
    const uint64_t *bits = nullptr;
    int64_t n, nvals;
    gb_bitmap_view bv;
    gb_csr_view cv;
    if (A->kind == GB_KIND_MATRIX) {
        gb_get_csr(cv, A);
        vals = gb_view_vals_as(cv, code, s);
        iso = cv.iso;
        nvals = cv.nvals;
        n = nvals;
    } else {
        gb_get_bitmap(bv, A);
        vals = gb_bitmap_vals_as(bv, code, s);
        iso = bv.iso;
        bits = bv.bits;
        n = bv.n;
        nvals = n;
    }
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(256, (n + 255) / 256));
    bool any = false;
    gb_with_type(code, [&](auto z) {
        using T = decltype(z);
        T *part = s.get<T>(nb);
        int *pf = s.get<int>(nb);
        hipLaunchKernelGGL(k_reduce_partial<T>, dim3(nb), dim3(256), 0, gb_stream(), monoid->mcode, (const T *)vals,
                           iso, nvals, bits, n, part, pf);
        GB_LAUNCH_CHECK();
        std::vector<char> hpb(nb * sizeof(T));
        std::vector<int> hf(nb);
        gb_copy_d2h(hpb.data(), part, nb * sizeof(T));
        gb_copy_d2h(hf.data(), pf, nb * sizeof(int));
        T acc = T();
        for (int b = 0; b < nb; b++)
            if (hf[b]) {
                T hv;
                memcpy(&hv, hpb.data() + b * sizeof(T), sizeof(T));
                acc = any ? gb_monoid<T>(monoid->mcode, acc, hv) : hv;
                any = true;
            }
        memcpy(out, &acc, sizeof(T));
    });
    return any;
}

// identity of a monoid (value written to *out)
static void monoid_identity(GrB_Monoid monoid, void *out) {
    int m = monoid->mcode;
    gb_with_type(monoid->type->code, [&](auto z) {
        using T = decltype(z);
        T v = T();
        switch (m) {
        case GBAMD_MON_TIMES: v = (T)1; break;
        case GBAMD_MON_MIN: v = gb_tmax<T>(); break;
        case GBAMD_MON_MAX: v = gb_tmin<T>(); break;
        case GBAMD_MON_LAND: case GBAMD_MON_LXNOR: v = (T)1; break;
        case GBAMD_MON_BAND: case GBAMD_MON_BXNOR:
            if constexpr (gb_traits<T>::is_int) v = (T)~(T)0;
            break;
        default: v = T(); break;
        }
        memcpy(out, &v, sizeof(T));
    });
}

// ================================================================== transpose
// T = a copy of a CSR view (transpose, matrix assign)
static void copy_csr_T(gb_mat_result &T, const gb_csr_view &v) {
    T = gb_new_mat_result(v.nrows, v.ncols, v.tcode, v.nvals, v.iso);
    gb_copy_d2d(T.rowptr, v.rowptr, (v.nrows + 1) * sizeof(int64_t));
    gb_copy_d2d(T.colidx, v.colidx, v.nvals * sizeof(int32_t));
    gb_copy_d2d(T.vals, v.vals, (v.iso ? 1 : v.nvals) * gb_type_size(v.tcode));
}
// the values, bitmap and count of T (n positions) = a copy of a bitmap view (vector assign)
static void copy_bitmap_T(gb_vec_result &T, const gb_bitmap_view &v, int64_t n) {
    T.iso = v.iso;
    T.bits = gb_malloc_n<uint64_t>(gb_words(n));
    gb_copy_d2d(T.bits, v.bits, gb_words(n) * sizeof(uint64_t));
    const size_t ts = gb_type_size(v.tcode);
    T.dense = gb_malloc((v.iso ? 1 : n) * ts);
    gb_copy_d2d(T.dense, v.vals, (v.iso ? 1 : n) * ts);
    T.d_nvals = gb_malloc_n<int64_t>(1);
    gb_bitmap_count(T.bits, n, T.d_nvals);
}

static void do_transpose(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GB_Obj *A, const gb_desc &d) {
    gb_check_binop(accum, true);
    gb_csr_view v;
    if (d.tran0) gb_get_csr(v, A);  // transpose of the transpose
    else gb_get_csc(v, A);
    gb_mat_result T;
    copy_csr_T(T, v);
    gb_writeback_matrix(C, T, M, d, accum);
}

// ================================================================== assign
// T for "x assigned at every index of I (GrB_ALL: all)": iso bitmap vector
static void scalar_vec_T(gb_vec_result &T, int64_t n, const GrB_Index *I, int64_t ni, const void *x, int code) {
    T = gb_new_vec_result(n, code, true);
    int64_t nw = gb_words(n);
    gb_copy_h2d(T.dense, x, gb_type_size(code));
    if (I == GrB_ALL) {
        std::vector<uint64_t> hb(nw, ~0ULL);
        if (n & 63) hb[nw - 1] = (1ULL << (n & 63)) - 1;
        gb_copy_h2d(T.bits, hb.data(), nw * sizeof(uint64_t));
        int64_t nn = n;
        gb_copy_h2d(T.d_nvals, &nn, sizeof(int64_t));
        gb_sync();
        return;
    }
    std::vector<uint64_t> hb(nw, 0);
    int64_t c = 0;
    gb_index_list L;
    gb_expand_indices(L, I, (GrB_Index)ni, n);
    for (int64_t i : L.idx) {
        uint64_t &w = hb[i >> 6];
        uint64_t b = 1ULL << (i & 63);
        if (!(w & b)) c++;
        w |= b;
    }
    gb_copy_h2d(T.bits, hb.data(), nw * sizeof(uint64_t));
    gb_copy_h2d(T.d_nvals, &c, sizeof(int64_t));
    gb_sync();
}

static GrB_BinaryOp second_of(int code) {
    void *h;
    int kind;
    std::string name = std::string("GrB_SECOND_") + gb_type_name(code);
    GxB_builtin_lookup(&h, &kind, name.c_str());
    return (GrB_BinaryOp)h;
}

// w<M, replace>(:) = x with no accumulator, in place: one pass over the bitmap,
// values written only where the mask selects (BFS level stamping,
// notebooks/Example B.1 cell 8: v[:](mask=q.V) << d).  Waves whose 64 mask bits
// select nothing (and do not replace) leave their word untouched.
template <class T>
__global__ __launch_bounds__(OPS_BLOCK) void k_assign_all_scalar(
    int64_t n, uint64_t *__restrict__ cbits, T *__restrict__ cvals, const uint64_t *__restrict__ mbits, bool mcomp,
    const void *miso, int miso_code, bool replace, T x, unsigned long long *__restrict__ count,
    unsigned long long *__restrict__ gst) {
    // value mask over an iso vector: the mask is its structure if the value is true, else empty
    const bool iso_true = miso ? gb_dyn_nonzero(miso, miso_code) : true;
    long long delta = 0;  // change of nvals(C); added to the count C already holds
    for (int64_t base = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~63LL; base < n;
         base += (int64_t)gridDim.x * blockDim.x) {
        const int lane = threadIdx.x & 63;
        const int64_t w = base >> 6;
        const int64_t i = base + lane;
        uint64_t mword = (mbits && iso_true) ? mbits[w] : 0;
        if (mbits && !mcomp && mword == 0 && !replace) continue;
        const uint64_t cword = cbits[w];
        bool inr = i < n;
        bool m = inr && (mbits ? ((((mword >> lane) & 1ULL) != 0) != mcomp) : !mcomp);
        bool c = (cword >> lane) & 1ULL;
        if (m) cvals[i] = x;
        bool have = m || (!replace && c && inr);
        unsigned long long word = __ballot(have);
        if (lane == 0) {
            if (word != cword) cbits[w] = word;
            delta += (long long)__popcll(word) - (long long)__popcll(cword);
        }
    }
    gb_grid_add(delta, count, gst);
}

// w<M>(:) = x, M a plain (non-complemented) mask, no replace: a wave takes 16
// mask words per step, one per lane (each lane updates its presence word);
// then the selected values of each non-zero word are written by the whole
// wave, one lane per position (coalesced stores).
template <class T>
__global__ __launch_bounds__(OPS_BLOCK) void k_assign_mask_words(int64_t nwords, uint64_t *__restrict__ cbits,
                                                                 T *__restrict__ cvals,
                                                                 const uint64_t *__restrict__ mbits, const void *miso,
                                                                 int miso_code, T x,
                                                                 unsigned long long *__restrict__ count,
                                                                 unsigned long long *__restrict__ gst) {
    const bool iso_true = miso ? gb_dyn_nonzero(miso, miso_code) : true;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    long long delta = 0;
    if (iso_true) {
        for (int64_t base = wave * 16; base < nwords; base += nwaves * 16) {
            const int64_t w = base + lane;
            const uint64_t m = (lane < 16 && w < nwords) ? mbits[w] : 0;
            if (m) {
                const uint64_t c = cbits[w], nwd = c | m;
                if (nwd != c) cbits[w] = nwd;
                delta += (long long)__popcll(nwd) - (long long)__popcll(c);
            }
            unsigned long long nz = __ballot(m != 0);
            while (nz) {
                const int l = __ffsll(nz) - 1;
                nz &= nz - 1;
                const uint64_t mw = __shfl(m, l, 64);
                if ((mw >> lane) & 1ULL) cvals[((base + l) << 6) + lane] = x;
            }
        }
    }
    gb_grid_add(delta, count, gst);
}

// make a vector's value array writable in place (non-iso, allocated) and its count present
void gb_make_values_writable(GB_Obj *w) {
    const int64_t n = w->nrows;
    const size_t ts = w->type->size;
    if (!w->dense) {
        w->dense = gb_malloc(n * ts);
        w->iso = false;
    } else if (w->iso) {
        void *full = gb_expand_iso(w->dense, ts, n);
        gb_free(w->dense);
        w->dense = full;
        w->iso = false;
    }
    if (!w->d_nvals) {
        w->d_nvals = gb_malloc_n<int64_t>(1);
        gb_memset(w->d_nvals, 0, sizeof(int64_t));
    }
}

bool gb_assign_all_scalar_fast(GB_Obj *w, GB_Obj *mask, const char *xc, const gb_desc &d) {
    if (w->kind == GB_KIND_MATRIX) return false;
    const int64_t n = w->nrows;
    const size_t ts = w->type->size;
    gb_vmask m;
    gb_make_vmask(m, mask, d, n, true);
    if (!m.bits && !m.comp) {
        // no mask: w becomes full and iso x
        int64_t nw = gb_words(n);
        uint64_t *bits = gb_malloc_n<uint64_t>(nw);
        gb_memset(bits, 0xff, nw * sizeof(uint64_t));
        if (n & 63) {
            uint64_t last = (1ULL << (n & 63)) - 1;
            gb_copy_h2d(bits + nw - 1, &last, sizeof(last));
        }
        void *dense = gb_malloc(ts);
        gb_copy_h2d(dense, xc, ts);
        int64_t *cnt = gb_malloc_n<int64_t>(1);
        gb_copy_h2d(cnt, &n, sizeof(int64_t));
        gb_sync();  // the host-side sources above live on this stack frame
        gb_install_bitmap(w, n, bits, dense, true, cnt);
        return true;
    }
    gb_make_values_writable(w);
    unsigned grid = (unsigned)std::min<int64_t>((n + OPS_BLOCK - 1) / OPS_BLOCK, 1024);
    gb_with_type(w->type->code, [&](auto z) {
        using T = decltype(z);
        T xv;
        memcpy(&xv, xc, sizeof(T));
        if (n && m.bits && !m.comp && !d.replace)
            hipLaunchKernelGGL(k_assign_mask_words<T>,
                               dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((gb_words(n) + 63) / 64, 2048))),
                               dim3(OPS_BLOCK), 0, gb_stream(), gb_words(n), w->bits, (T *)w->dense, m.bits, m.iso_val,
                               m.iso_code, xv, (unsigned long long *)w->d_nvals, gb_device_state());
        else if (n)
            hipLaunchKernelGGL(k_assign_all_scalar<T>, dim3(grid), dim3(OPS_BLOCK), 0, gb_stream(), n, w->bits,
                               (T *)w->dense, m.bits, m.comp, m.iso_val, m.iso_code, d.replace, xv,
                               (unsigned long long *)w->d_nvals, gb_device_state());
    });
    GB_LAUNCH_CHECK();
    w->nvals_valid = false;
    w->hint_valid = false;
    return true;
}

void gb_vector_assign_scalar(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, const void *x, int xcode,
                             const GrB_Index *I, int64_t ni, const gb_desc &d) {
    gb_check_binop(accum, true);
    GB_REQUIRE(w->kind != GB_KIND_MATRIX || w->ncols == 1, GrB_DIMENSION_MISMATCH, "not a vector");
    int ct = w->type->code;
    char xc[16] = {0};
    gb_cast_scalar(xc, ct, x, xcode);
    // the BFS level stamp is deferred (gb_bfs_loop.hip); its mask may then stay a pending root
    if (I == GrB_ALL && !accum && gb_stamp_try_defer(w, mask, xc, d)) return;
    // not deferred: the assign reads a pending root (the caller resolved everything else)
    if (g_deferred.load(std::memory_order_acquire)) gb_deferred_resolve(GB_DEFER_SPEC | GB_DEFER_STAMP, nullptr);
    if (I == GrB_ALL && !accum && gb_assign_all_scalar_fast(w, mask, xc, d)) return;
    gb_vec_result T;
    scalar_vec_T(T, w->nrows, I, ni, xc, ct);
    GrB_BinaryOp acc = accum;
    if (I != GrB_ALL && !acc) acc = second_of(ct);  // outside I, C is kept
    gb_writeback_vector(w, T, mask, d, acc, false);
}

static void matrix_assign_scalar(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, const void *x, int xcode,
                                 const GrB_Index *I, int64_t ni, const GrB_Index *J, int64_t nj, const gb_desc &d) {
    gb_check_binop(accum, true);
    int ct = C->type->code;
    char xc[16] = {0};
    gb_cast_scalar(xc, ct, x, xcode);
    int64_t nr = C->nrows, nc = gb_ncols_of(C);
    gb_index_list LI, LJ;
    gb_expand_indices(LI, I, (GrB_Index)ni, nr);
    gb_expand_indices(LJ, J, (GrB_Index)nj, nc);
    std::vector<int64_t> rows, cols;
    if (LI.all) {
        rows.resize(nr);
        for (int64_t i = 0; i < nr; i++) rows[i] = i;
    } else rows = LI.idx;
    if (LJ.all) {
        cols.resize(nc);
        for (int64_t j = 0; j < nc; j++) cols[j] = j;
    } else cols = LJ.idx;
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    int64_t nz = (int64_t)rows.size() * (int64_t)cols.size();
    std::vector<int64_t> rp(nr + 1, 0);
    for (auto r : rows) rp[r + 1] = (int64_t)cols.size();
    for (int64_t i = 0; i < nr; i++) rp[i + 1] += rp[i];
    std::vector<int32_t> ci(nz);
    for (size_t a = 0; a < rows.size(); a++)
        for (size_t b = 0; b < cols.size(); b++) ci[a * cols.size() + b] = (int32_t)cols[b];
    gb_mat_result T = gb_new_mat_result(nr, nc, ct, nz, true);
    gb_copy_h2d(T.rowptr, rp.data(), (nr + 1) * sizeof(int64_t));
    gb_copy_h2d(T.colidx, ci.data(), nz * sizeof(int32_t));
    gb_copy_h2d(T.vals, xc, gb_type_size(ct));
    gb_sync();
    GrB_BinaryOp acc = accum;
    if ((I != GrB_ALL || J != GrB_ALL) && !acc) acc = second_of(ct);
    gb_writeback_matrix(C, T, M, d, acc);
}

// ================================================================== C API
// ================================================================== apply
// z = op(x) (kind 0), op(s, x) (kind 1, BinaryOp1st), op(x, s) (kind 2, BinaryOp2nd)
// over the n stored values (n = 1 for iso inputs): structure is not touched.
template <class X, class Z>
__global__ void k_apply(int64_t n, int kind, int op, const X *__restrict__ in, X s, Z *__restrict__ out) {
    GB_GRID_LOOP(i, n) {
        X x = in[i];
        if (kind == 0) out[i] = gb_cast<Z, X>(gb_unop<X>(op, x));
        else if (kind == 1) out[i] = gb_binop_z<X, Z>(op, s, x, 0, 0, 0);
        else out[i] = gb_binop_z<X, Z>(op, x, s, 0, 0, 0);
    }
}

// kind 0: uop; kind 1/2: bop with the bound scalar *sval (type scode)
static void do_apply(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, int kind, GrB_UnaryOp uop, GrB_BinaryOp bop,
                     const void *sval, int scode, GB_Obj *A, const gb_desc &d) {
    gb_check_binop(accum, true);
    int xcode, zcode, opcode;
    if (kind == 0) {
        GB_REQUIRE(uop, GrB_NULL_POINTER, "operator is NULL");
        GB_REQUIRE(uop->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid operator");
        xcode = uop->xtype->code;
        zcode = uop->ztype->code;
        opcode = uop->opcode;
    } else {
        gb_check_binop(bop, false);
        GB_REQUIRE(bop->xtype != nullptr, GrB_NOT_IMPLEMENTED, "positional operator in apply");
        xcode = bop->xtype->code;
        zcode = bop->ztype->code;
        opcode = bop->opcode;
    }
    // the bound scalar, cast to the operator's input type
    char sx[16] = {0};
    if (kind != 0) gb_cast_scalar(sx, xcode, sval, scode);
    auto launch = [&](int64_t n, const void *in, void *out) {
        gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
            using X = decltype(x);
            using Z = decltype(z);
            X s;
            memcpy(&s, sx, sizeof(X));
            if (n)
                hipLaunchKernelGGL((k_apply<X, Z>), dim3(gb_grid(n, OPS_BLOCK, OPS_GRID_CAP)), dim3(OPS_BLOCK), 0,
                                   gb_stream(), n, kind, opcode, (const X *)in, s, (Z *)out);
        });
        GB_LAUNCH_CHECK();
    };
    const size_t zs = gb_type_size(zcode);
    if (C->kind != GB_KIND_MATRIX) {
        GB_REQUIRE(A->nrows == C->nrows && gb_ncols_of(A) == 1, GrB_DIMENSION_MISMATCH, "vector sizes do not match");
        gb_bitmap_view uv;
        gb_get_bitmap(uv, A);
        gb_scratch s;
        const void *xin = gb_bitmap_vals_as(uv, xcode, s);
        gb_vec_result T = gb_new_vec_result(uv.n, zcode, uv.iso);
        const int64_t nw = gb_words(uv.n);
        if (nw) gb_copy_d2d(T.bits, uv.bits, nw * sizeof(uint64_t));
        launch(uv.iso ? 1 : uv.n, xin, T.dense);
        if (uv.count) gb_copy_d2d(T.d_nvals, uv.count, sizeof(int64_t));
        else gb_bitmap_count(T.bits, T.n, T.d_nvals);
        gb_writeback_vector(C, T, M, d, accum, false);
        return;
    }
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    GB_REQUIRE(v.nrows == C->nrows && v.ncols == C->ncols, GrB_DIMENSION_MISMATCH, "matrix dimensions do not match");
    gb_scratch s;
    const void *xin = gb_view_vals_as(v, xcode, s);
    gb_mat_result T = gb_new_mat_result(v.nrows, v.ncols, zcode, v.nvals, v.iso);
    gb_copy_d2d(T.rowptr, v.rowptr, (v.nrows + 1) * sizeof(int64_t));
    if (v.nvals) gb_copy_d2d(T.colidx, v.colidx, v.nvals * sizeof(int32_t));
    launch(v.iso ? (v.nvals ? 1 : 0) : v.nvals, xin, T.vals);
    gb_writeback_matrix(C, T, M, d, accum);
}

// ================================================================== reduce to vector
static GrB_BinaryOp first_of(int code) {
    void *h;
    int kind;
    std::string name = std::string("GrB_FIRST_") + gb_type_name(code);
    GxB_builtin_lookup(&h, &kind, name.c_str());
    return (GrB_BinaryOp)h;
}

static void do_reduce_rows(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, GrB_Monoid monoid, GB_Obj *A,
                           const gb_desc &d) {
    GB_REQUIRE(monoid, GrB_NULL_POINTER, "monoid is NULL");
    GB_REQUIRE(monoid->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid monoid");
    GB_REQUIRE(A->kind == GB_KIND_MATRIX, GrB_INVALID_OBJECT, "reduce input must be a matrix");
    const int code = monoid->type->code;
    // w = A' (monoid.FIRST) ones: the product is A'(i,k); the iso-full vector only supplies structure
    GB_Semiring_opaque sr{GB_MAGIC, monoid, first_of(code), "reduce", false};
    const int64_t k = d.tran0 ? A->nrows : A->ncols;
    GrB_Vector u = nullptr;
    GrB_Info info = GrB_Vector_new(&u, monoid->type, (GrB_Index)k);
    GB_REQUIRE(info == GrB_SUCCESS, info, "cannot allocate the reduction vector");
    struct Free {
        GrB_Vector *u;
        ~Free() { GrB_Vector_free(u); }
    } fr{&u};
    char one[16] = {0};
    gb_with_type(code, [&](auto z) {
        using Z = decltype(z);
        Z v = (Z)1;
        memcpy(one, &v, sizeof(Z));
    });
    gb_vector_assign_scalar(OBJ(u), nullptr, nullptr, one, code, GrB_ALL, k, gb_desc());
    gb_desc dd = d;
    dd.tran1 = false;
    gb_do_spmv(w, mask, accum, &sr, A, OBJ(u), dd, false);
}

static GrB_Monoid monoid_of_binop(GrB_BinaryOp op) {
    gb_check_binop(op, false);
    GB_REQUIRE(op->xtype != nullptr && op->xtype == op->ztype, GrB_DOMAIN_MISMATCH,
               "reduce requires a BinaryOp that is a monoid");
    static const struct {
        int opcode;
        const char *pre, *mid;
    } tab[] = {{GBAMD_OP_PLUS, "GrB_PLUS_MONOID_", nullptr},   {GBAMD_OP_TIMES, "GrB_TIMES_MONOID_", nullptr},
               {GBAMD_OP_MIN, "GrB_MIN_MONOID_", nullptr},     {GBAMD_OP_MAX, "GrB_MAX_MONOID_", nullptr},
               {GBAMD_OP_ANY, "GxB_ANY_", "_MONOID"},          {GBAMD_OP_LOR, "GrB_LOR_MONOID_", nullptr},
               {GBAMD_OP_LAND, "GrB_LAND_MONOID_", nullptr},   {GBAMD_OP_LXOR, "GrB_LXOR_MONOID_", nullptr},
               {GBAMD_OP_LXNOR, "GrB_LXNOR_MONOID_", nullptr}, {GBAMD_OP_BOR, "GxB_BOR_", "_MONOID"},
               {GBAMD_OP_BAND, "GxB_BAND_", "_MONOID"},        {GBAMD_OP_BXOR, "GxB_BXOR_", "_MONOID"},
               {GBAMD_OP_BXNOR, "GxB_BXNOR_", "_MONOID"}};
    for (auto &t : tab) {
        if (t.opcode != op->opcode) continue;
        std::string name = std::string(t.pre) + gb_type_name(op->ztype->code) + (t.mid ? t.mid : "");
        void *h = nullptr;
        int kind = -1;
        if (GxB_builtin_lookup(&h, &kind, name.c_str()) == GrB_SUCCESS && kind == 2) return (GrB_Monoid)h;
    }
    gb_throw(GrB_DOMAIN_MISMATCH, "reduce requires a BinaryOp that is a monoid");
    return nullptr;
}

extern "C" {

GrB_Info GrB_mxm(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Semiring op,
                 const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        const gb_desc d = gb_read_desc(desc);
        if (gb_colbits_mxm(gb_obj_check_raw(C), gb_obj_check_raw(Mask, true), accum, op, gb_obj_check_raw(A),
                           gb_obj_check_raw(B), d))
            return;
        do_mxm(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), gb_obj_check(B), d);
    });
}

GrB_Info GrB_Matrix_eWiseMult_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                       const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B,
                                       const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        do_ewise(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), gb_obj_check(B),
                 gb_read_desc(desc), false);
    });
}
GrB_Info GrB_Vector_eWiseMult_BinaryOp(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                                       const GrB_BinaryOp op, const GrB_Vector u, const GrB_Vector v,
                                       const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        do_ewise(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(u), gb_obj_check(v),
                 gb_read_desc(desc), false);
    });
}
GrB_Info GrB_Matrix_eWiseAdd_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                      const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B,
                                      const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        do_ewise(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), gb_obj_check(B),
                 gb_read_desc(desc), true);
    });
}
GrB_Info GrB_Vector_eWiseAdd_BinaryOp(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                                      const GrB_BinaryOp op, const GrB_Vector u, const GrB_Vector v,
                                      const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        do_ewise(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(u), gb_obj_check(v),
                 gb_read_desc(desc), true);
    });
}

GrB_Info GrB_transpose(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A,
                       const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        do_transpose(gb_obj_check(C), gb_obj_check(Mask, true), accum, gb_obj_check(A), gb_read_desc(desc));
    });
}

// w(I) = u without accum replaces the region: entries of w at I (where the mask selects)
// that u does not hold are deleted.  Clears those bits before the merge with accum SECOND.
__global__ void k_clear_region(int64_t nw, uint64_t *__restrict__ wbits, const uint64_t *__restrict__ rbits,
                               const uint64_t *__restrict__ mbits, bool mcomp) {
    GB_GRID_LOOP(k, nw) {
        uint64_t sel = mbits ? (mcomp ? ~mbits[k] : mbits[k]) : ~0ULL;
        wbits[k] &= ~(rbits[k] & sel);
    }
}

static void vector_clear_region(GB_Obj *W, const gb_index_list &L, GB_Obj *M, const gb_desc &d) {
    const int64_t n = W->nrows, nw = gb_words(n);
    GB_REQUIRE(W->kind != GB_KIND_MATRIX, GrB_NOT_IMPLEMENTED, "index-list assign into an n x 1 matrix");
    if (nw == 0) return;
    std::vector<uint64_t> hr(nw, 0);
    for (int64_t i : L.idx) hr[i >> 6] |= 1ULL << (i & 63);
    gb_scratch s;
    uint64_t *r = s.get<uint64_t>(nw);
    gb_copy_h2d(r, hr.data(), nw * sizeof(uint64_t));
    gb_vmask m;
    gb_make_vmask(m, M, d, n);
    hipLaunchKernelGGL(k_clear_region, dim3(gb_grid(nw, OPS_BLOCK, OPS_GRID_CAP)), dim3(OPS_BLOCK), 0, gb_stream(), nw,
                       W->bits, r, m.bits, m.comp);
    GB_LAUNCH_CHECK();
    gb_vec_recount(W);
    gb_sync();
}

GrB_Info GrB_Vector_assign(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u,
                           const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_Obj *W = gb_obj_check(w), *U = gb_obj_check(u);
        gb_desc d = gb_read_desc(desc);
        gb_check_binop(accum, true);
        int64_t n = W->nrows;
        gb_vec_result T;
        T.n = n;
        T.tcode = U->type->code;
        if (I == GrB_ALL) {
            GB_REQUIRE(U->nrows == n, GrB_DIMENSION_MISMATCH, "u size does not match w");
            gb_bitmap_view uv;
            gb_get_bitmap(uv, U);
            copy_bitmap_T(T, uv, n);
            gb_writeback_vector(W, T, gb_obj_check(mask, true), d, accum, false);
            return;
        }
        // index list: w(I[k]) = u(k)
        gb_index_list L;
        gb_expand_indices(L, I, ni, n);
        GB_REQUIRE(U->nrows == L.n, GrB_DIMENSION_MISMATCH, "u size does not match the index list");
        int64_t unv = gb_nvals(U);
        std::vector<GrB_Index> ui(unv);
        std::vector<char> ux(unv * U->type->size);
        {
            GrB_Index nv = unv;
            gb_extract_tuples(U, ui.data(), nullptr, ux.data(), U->type->code, &nv);
        }
        GB_Obj *Tv = gb_new_object(GB_KIND_VECTOR, U->type, n, 1);
        std::vector<GrB_Index> wi(unv);
        for (int64_t q = 0; q < unv; q++) {
            GB_REQUIRE(ui[q] < (GrB_Index)L.n, GrB_INDEX_OUT_OF_BOUNDS, "index out of bounds");
            wi[q] = (GrB_Index)L.idx[ui[q]];
        }
        try {
            gb_build(Tv, wi.data(), nullptr, ux.data(), U->type->code, false, unv, nullptr);
        } catch (...) {
            GrB_Vector tv = (GrB_Vector)Tv;
            GrB_Vector_free(&tv);
            throw;
        }
        gb_bitmap_view tvw;
        gb_get_bitmap(tvw, Tv);
        copy_bitmap_T(T, tvw, n);
        GrB_Vector tv = (GrB_Vector)Tv;
        GrB_Vector_free(&tv);
        GB_Obj *Mo = gb_obj_check(mask, true);
        // w(w.S)[I] = u / w(w.V)[I] = u: the region clear below edits w's bitmap, which IS the
        // mask; the writeback must see the mask as it was before the clear, so take a copy
        struct mask_copy {
            GrB_Vector h = nullptr;
            ~mask_copy() { if (h) GrB_Vector_free(&h); }
        } mc;
        if (!accum && Mo == W) {
            GB_REQUIRE(GrB_Vector_dup(&mc.h, mask) == GrB_SUCCESS, GrB_OUT_OF_MEMORY, "mask copy");
            Mo = gb_obj_check(mc.h);
        }
        if (!accum) vector_clear_region(W, L, Mo, d);
        gb_writeback_vector(W, T, Mo, d, accum ? accum : second_of(W->type->code), false);
    });
}

GrB_Info GrB_Matrix_assign(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A,
                           const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj,
                           const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C), *Ao = gb_obj_check(A);
        gb_desc d = gb_read_desc(desc);
        GB_REQUIRE(I == GrB_ALL && J == GrB_ALL, GrB_NOT_IMPLEMENTED, "Matrix_assign supports GrB_ALL only");
        gb_csr_view v;
        if (d.tran0) gb_get_csc(v, Ao);
        else gb_get_csr(v, Ao);
        GB_REQUIRE(v.nrows == Co->nrows && v.ncols == gb_ncols_of(Co), GrB_DIMENSION_MISMATCH, "dimension mismatch");
        gb_mat_result T;
        copy_csr_T(T, v);
        gb_writeback_matrix(Co, T, gb_obj_check(Mask, true), d, accum);
    });
}

GrB_Info GrB_Matrix_reduce_Monoid_Scalar(GrB_Scalar s, const GrB_BinaryOp accum, const GrB_Monoid monoid,
                                         const GrB_Matrix A, const GrB_Descriptor desc) {
    (void)desc;
    return gb_api(OBJ(s), [&] {
        GB_Obj *S = gb_obj_check(s);
        char v[16];
        bool any = reduce_values(gb_obj_check(A), monoid, v);
        gb_vec_result T = gb_new_vec_result(1, monoid->type->code, true);
        uint64_t b = any ? 1 : 0;
        gb_copy_h2d(T.bits, &b, sizeof(b));
        gb_copy_h2d(T.dense, v, gb_type_size(T.tcode));
        int64_t nn = any ? 1 : 0;
        gb_copy_h2d(T.d_nvals, &nn, sizeof(nn));
        gb_sync();
        gb_writeback_vector(S, T, nullptr, gb_desc(), accum, false);
    });
}
GrB_Info GrB_Vector_reduce_Monoid_Scalar(GrB_Scalar s, const GrB_BinaryOp accum, const GrB_Monoid monoid,
                                         const GrB_Vector u, const GrB_Descriptor desc) {
    return GrB_Matrix_reduce_Monoid_Scalar(s, accum, monoid, (GrB_Matrix)u, desc);
}
GrB_Info GrB_Matrix_reduce_Monoid(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                                  const GrB_Monoid monoid, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        do_reduce_rows(gb_obj_check(w), gb_obj_check(mask, true), accum, monoid, gb_obj_check(A),
                       gb_read_desc(desc));
    });
}
GrB_Info GrB_Matrix_reduce_BinaryOp(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                                    const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        do_reduce_rows(gb_obj_check(w), gb_obj_check(mask, true), accum, monoid_of_binop(op), gb_obj_check(A),
                       gb_read_desc(desc));
    });
}
GrB_Info GrB_Vector_apply(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_UnaryOp op,
                          const GrB_Vector u, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        do_apply(gb_obj_check(w), gb_obj_check(mask, true), accum, 0, op, nullptr, nullptr, 0, gb_obj_check(u),
                 gb_read_desc(desc));
    });
}
GrB_Info GrB_Matrix_apply(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_UnaryOp op,
                          const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        do_apply(gb_obj_check(C), gb_obj_check(Mask, true), accum, 0, op, nullptr, nullptr, 0, gb_obj_check(A),
                 gb_read_desc(desc));
    });
}
GrB_Info GrB_Semiring_new(GrB_Semiring *semiring, GrB_Monoid add, GrB_BinaryOp multiply) {
    if (!semiring || !add || !multiply) return GrB_NULL_POINTER;
    if (add->magic != GB_MAGIC || multiply->magic != GB_MAGIC) return GrB_UNINITIALIZED_OBJECT;
    if (multiply->ztype != add->type) return GrB_DOMAIN_MISMATCH;
    GB_Semiring_opaque *s = new (std::nothrow) GB_Semiring_opaque{GB_MAGIC, add, multiply, "user_semiring", true};
    if (!s) return GrB_OUT_OF_MEMORY;
    *semiring = s;
    return GrB_SUCCESS;
}

#define GB_DEFINE_TYPED_OPS(T, ctype)                                                                          \
    GrB_Info GrB_Vector_assign_##T(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, ctype x,   \
                                   const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc) {            \
        GB_HPROF(8, "GrB_Vector_assign scalar");                                                             \
        GrB_Info info = GrB_SUCCESS; /* the level stamp a speculation predicted is already carried out */    \
        if (gb_deferred_absorb_assign(w, mask, accum, &x, GBAMD_T_##T, I, ni, desc, &info)) return info;     \
        /* a deferred stamp whose mask is a pending root keeps it pending */                                 \
        return gb_api_impl<GB_DEFER_ROOT>(OBJ(w), [&] {                                                      \
            gb_vector_assign_scalar(gb_obj_check(w), gb_obj_check(mask, true), accum, &x, GBAMD_T_##T, I,    \
                                    (int64_t)ni, gb_read_desc(desc));                                        \
        }, __func__);                                                                                        \
    }                                                                                                        \
    GrB_Info GrB_Matrix_assign_##T(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, ctype x,   \
                                   const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj,       \
                                   const GrB_Descriptor desc) {                                              \
        return gb_api(OBJ(C), [&] {                                                                          \
            const gb_desc d = gb_read_desc(desc);                                                            \
            if (gb_colbits_assign_scalar(gb_obj_check_raw(C), gb_obj_check_raw(Mask, true), accum, &x,       \
                                         GBAMD_T_##T, I, J, d))                                              \
                return;                                                                                      \
            GB_Obj *Co = gb_obj_check(C);                                                                    \
            if (Co->kind != GB_KIND_MATRIX)                                                                  \
                gb_vector_assign_scalar(Co, gb_obj_check(Mask, true), accum, &x, GBAMD_T_##T, I, (int64_t)ni, \
                                        gb_read_desc(desc));                                                 \
            else                                                                                             \
                matrix_assign_scalar(Co, gb_obj_check(Mask, true), accum, &x, GBAMD_T_##T, I, (int64_t)ni, J, \
                                     (int64_t)nj, gb_read_desc(desc));                                       \
        });                                                                                                  \
    }                                                                                                        \
    GrB_Info GrB_Vector_reduce_##T(ctype *c, const GrB_BinaryOp accum, const GrB_Monoid monoid,              \
                                   const GrB_Vector u, const GrB_Descriptor desc) {                          \
        (void)desc;                                                                                          \
        if (!c) return GrB_NULL_POINTER;                                                                     \
        return gb_api(OBJ(u), [&] {                                                                          \
            char v[16];                                                                                      \
            GB_REQUIRE(monoid && monoid->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid monoid");     \
            if (!reduce_values(gb_obj_check(u), monoid, v)) monoid_identity(monoid, v);                      \
            ctype r;                                                                                         \
            gb_with_type(monoid->type->code, [&](auto z) {                                                   \
                using S = decltype(z);                                                                       \
                S sv;                                                                                        \
                memcpy(&sv, v, sizeof(S));                                                                   \
                r = gb_cast<ctype, S>(sv);                                                                   \
            });                                                                                              \
            if (accum) {                                                                                     \
                gb_check_binop(accum, false);                                                                   \
                r = gb_binop<ctype>(accum->opcode, *c, r);                                                   \
            }                                                                                                \
            *c = r;                                                                                          \
        });                                                                                                  \
    }                                                                                                        \
    GrB_Info GrB_Matrix_reduce_##T(ctype *c, const GrB_BinaryOp accum, const GrB_Monoid monoid,              \
                                   const GrB_Matrix A, const GrB_Descriptor desc) {                          \
        return GrB_Vector_reduce_##T(c, accum, monoid, (GrB_Vector)A, desc);                                 \
    }                                                                                                        \
    GrB_Info GrB_Vector_apply_BinaryOp1st_##T(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,  \
                                              const GrB_BinaryOp op, ctype x, const GrB_Vector u,            \
                                              const GrB_Descriptor desc) {                                   \
        return gb_api(OBJ(w), [&] {                                                                          \
            do_apply(gb_obj_check(w), gb_obj_check(mask, true), accum, 1, nullptr, op, &x, GBAMD_T_##T,      \
                     gb_obj_check(u), gb_read_desc(desc));                                                   \
        });                                                                                                  \
    }                                                                                                        \
    GrB_Info GrB_Vector_apply_BinaryOp2nd_##T(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,  \
                                              const GrB_BinaryOp op, const GrB_Vector u, ctype y,            \
                                              const GrB_Descriptor desc) {                                   \
        return gb_api(OBJ(w), [&] {                                                                          \
            do_apply(gb_obj_check(w), gb_obj_check(mask, true), accum, 2, nullptr, op, &y, GBAMD_T_##T,      \
                     gb_obj_check(u), gb_read_desc(desc));                                                   \
        });                                                                                                  \
    }                                                                                                        \
    GrB_Info GrB_Matrix_apply_BinaryOp1st_##T(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,  \
                                              const GrB_BinaryOp op, ctype x, const GrB_Matrix A,            \
                                              const GrB_Descriptor desc) {                                   \
        return gb_api(OBJ(C), [&] {                                                                          \
            do_apply(gb_obj_check(C), gb_obj_check(Mask, true), accum, 1, nullptr, op, &x, GBAMD_T_##T,      \
                     gb_obj_check(A), gb_read_desc(desc));                                                   \
        });                                                                                                  \
    }                                                                                                        \
    GrB_Info GrB_Matrix_apply_BinaryOp2nd_##T(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,  \
                                              const GrB_BinaryOp op, const GrB_Matrix A, ctype y,            \
                                              const GrB_Descriptor desc) {                                   \
        return gb_api(OBJ(C), [&] {                                                                          \
            do_apply(gb_obj_check(C), gb_obj_check(Mask, true), accum, 2, nullptr, op, &y, GBAMD_T_##T,      \
                     gb_obj_check(A), gb_read_desc(desc));                                                   \
        });                                                                                                  \
    }

GB_FOR_EACH_TYPE(GB_DEFINE_TYPED_OPS)

}  // extern "C"
