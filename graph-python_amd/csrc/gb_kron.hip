// gb_kron.hip -- GrB_kronecker: C<M> = accum(C, kron(A', B')).
//   GrB_Matrix_kronecker_{BinaryOp,Monoid,Semiring}   reference core/matrix.py:2253-2292
//
// A' is m x n, B' is p x q; every pair of stored entries gives
//   T(iA p + iB, jA q + jB) = op(A'(iA, jA), B'(iB, jB)),
// nvals(A) nvals(B) entries: a stream of stores read from two small, heavily reused inputs.
// Output row (iA, iB) is lenA(iA) shifted copies of row iB of B', so the row pointer is a
// closed form -- no counting pass, no scan, no atomics, no host read:
//   k_kron_rowptr   rowptrT[iA p + iB] = rowptrA[iA] nvals(B) + lenA(iA) rowptrB[iB]
//   k_kron_fill     entry-parallel on the output (an R-MAT hub row times a hub row is millions
//                   of entries in one output row): a wave owns a contiguous run of chunks of
//                   KRON_CHUNK output positions, lane l of step u fills position
//                   p0 + 64 u + l, so stores are coalesced and columns ascend within a row
//                   with no sort.  The rows of a chunk are found in rowptrT with the helpers
//                   k_select_mark uses (gb_wave_upper, gb_count_bounds of gb_device.cuh): the
//                   wave bounds the chunk's first and last row, lane l then owns row rlo - 1 + l and
//                   does that row's divides once -- row -> (iA, iB), and the A entry / B
//                   offset of the row's first position inside the chunk.  An entry at
//                   distance d < KRON_CHUNK from there is A entry + (rb + d) / lenB, B entry
//                   (rb + d) % lenB with rb < lenB: a quotient of at most KRON_CHUNK, taken
//                   with the row's float reciprocal and one correction step.  A chunk with
//                   64 or more row boundaries (rows of under 8 entries on average) lets
//                   every lane search and divide for itself.  The output is written once and
//                   not read back by the call: its stores are nontemporal (1.39 -> 1.26 ms
//                   for the 645 M-entry square of DESIGN section 4).
//   k_kron_rows     kron_method = 1: one thread per output row, nested loops over the row of
//                   A' and the row of B' -- the A/B baseline and the tests' second opinion.
// Values: FIRST / SECOND / ANY move the operand's values (cast to the operator's type) by size
// class; other operators compute gb_binop_z<X, Z>.  When the operator reads only iso operands
// T is iso: one value from a one-thread kernel, no value array.
// The write-back (mask, replace, accum, cast to C's type) is gb_writeback_matrix.
#include <algorithm>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define KRON_BLOCK 256
#define KRON_WPI 8      // 64-entry steps of a chunk
#define KRON_CHUNK 512  // output positions a wave fills per chunk
static_assert(KRON_CHUNK == KRON_WPI * 64, "a chunk is KRON_WPI wave-wide steps");

namespace {

// n / d and n % d (n >= 0, d > 0): the 32-bit divide when both fit, which is nearly always
GB_DEV void kron_divmod(int64_t n, int64_t d, int64_t *q, int64_t *r) {
    if ((((uint64_t)n | (uint64_t)d) >> 32) == 0) {
        const uint32_t qq = (uint32_t)n / (uint32_t)d;
        *q = qq;
        *r = (uint32_t)n - qq * (uint32_t)d;
    } else {
        const int64_t qq = n / d;
        *q = qq;
        *r = n - qq * d;
    }
}

// the entry-parallel kernel writes its output once, coalesced, and never reads it back: its
// stores are nontemporal (NT); the per-row kernel's scattered stores stay plain
template <bool NT, class T>
GB_DEV void kron_store(T *p, T v) {
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// ---- what a filled position t gets for its value, from A entry a and B entry b
template <class X, class Z>
struct kron_compute {
    int op;
    const X *ax, *bx;
    bool a_iso, b_iso, use_a, use_b;
    Z *oz;
    template <bool NT>
    GB_DEV void put(int64_t t, int64_t a, int64_t b) const {
        const X x = use_a ? ax[a_iso ? 0 : a] : X();
        const X y = use_b ? bx[b_iso ? 0 : b] : X();
        kron_store<NT, Z>(&oz[t], gb_binop_z<X, Z>(op, x, y, 0, 0, 0));
    }
};

// VS: bytes per value, 0 = no values to write (iso result)
template <int VS>
struct kron_move {
    const void *src;  // the values of A' (FIRST) or of B' (SECOND, ANY), one per entry
    bool from_b;
    void *dst;
    template <bool NT>
    GB_DEV void put(int64_t t, int64_t a, int64_t b) const {
        if (VS) {
            using W = gb_word_t<VS>;
            kron_store<NT, W>(&((W *)dst)[t], ((const W *)src)[from_b ? b : a]);
        }
    }
};

__global__ __launch_bounds__(KRON_BLOCK) void k_kron_rowptr(int64_t nrT, int64_t p, int64_t nvA, int64_t nvB,
                                                            const int64_t *__restrict__ rpA,
                                                            const int64_t *__restrict__ rpB,
                                                            int64_t *__restrict__ rpT) {
    // (the block size as a constant, not GB_GRID_LOOP's blockDim.x: two scalar registers apart)
    for (int64_t R = blockIdx.x * (int64_t)KRON_BLOCK + threadIdx.x; R <= nrT; R += (int64_t)gridDim.x * KRON_BLOCK) {
        if (R == nrT) {
            rpT[R] = nvA * nvB;
            continue;
        }
        int64_t iA, iB;
        kron_divmod(R, p, &iA, &iB);
        const int64_t a0 = rpA[iA];
        rpT[R] = a0 * nvB + (rpA[iA + 1] - a0) * rpB[iB];
    }
}

template <class X, class Z>
__global__ void k_kron_iso(int op, const X *ax, const X *bx, bool use_a, bool use_b, Z *oz) {
    oz[0] = gb_binop_z<X, Z>(op, use_a ? ax[0] : X(), use_b ? bx[0] : X(), 0, 0, 0);
}

// nvT > 0 positions, nrT = m p output rows, q = columns of B'
template <class V>
__global__ __launch_bounds__(KRON_BLOCK) void k_kron_fill(int64_t nvT, int64_t nrT, int64_t p, int64_t q,
                                                          const int64_t *__restrict__ rpT,
                                                          const int64_t *__restrict__ rpA,
                                                          const int32_t *__restrict__ ciA,
                                                          const int64_t *__restrict__ rpB,
                                                          const int32_t *__restrict__ ciB,
                                                          int32_t *__restrict__ oci, V vop) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * KRON_BLOCK) >> 6;
    const int64_t nchunks = (nvT + KRON_CHUNK - 1) / KRON_CHUNK;
    const int64_t per_wave = (nchunks + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)KRON_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, nchunks);
    int64_t next = -1;  // a lower bound of the next chunk's rlo (-1: not known yet)
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = g * KRON_CHUNK;
        const int64_t plast = min(p0 + KRON_CHUNK, nvT) - 1;
        // rows rlo - 1 .. rhi - 1 hold the chunk; rpT[rlo .. rhi) are the boundaries inside it
        const int64_t rlo = next < 0 ? gb_upper_bound(rpT, 1, nrT, p0) : gb_wave_upper(rpT, next, nrT, p0, lane);
        const int64_t rhi = gb_wave_upper(rpT, rlo, nrT, plast, lane);
        next = rhi;
        if (rhi - rlo < 64) {
            const int nb = (int)(rhi - rlo);
            // lane l <= nb owns row rlo - 1 + l: where it starts in the chunk (rel), the A entry
            // (ab) and B offset (rb) of that position, the B row's first entry (bb) and length (lb)
            int rel = INT32_MAX;
            int64_t ab = 0, bb = 0;
            uint32_t rb = 0, lb = 1;
            float rcp = 0.0f;
            if (lane <= nb) {
                const int64_t R = rlo - 1 + lane;
                const int64_t st = rpT[R];
                int64_t iA, iB;
                kron_divmod(R, p, &iA, &iB);
                const int64_t b0 = rpB[iB];
                const int64_t lenB = rpB[iB + 1] - b0;
                const int64_t first = max(st, p0);  // lane 0: st <= p0; the others: p0 < st <= plast
                rel = (int)(first - p0);
                int64_t qa = 0, r0 = 0;
                if (lenB > 0) kron_divmod(first - st, lenB, &qa, &r0);  // an empty row owns no position
                ab = rpA[iA] + qa;
                bb = b0;
                rb = (uint32_t)r0;
                lb = (uint32_t)lenB;
                rcp = __builtin_amdgcn_rcpf((float)lenB);
            }
            // an entry's row slot: the number of boundaries (lanes 1 .. nb) at or below it
            int slot[KRON_WPI];
            gb_count_bounds<KRON_WPI>(rel, 1, nb, lane, slot);
#pragma unroll
            for (int u = 0; u < KRON_WPI; u++) {
                const int o = u * 64 + lane;
                const int s = slot[u];
                const int srel = __shfl(rel, s);
                const uint32_t srb = __shfl(rb, s), slb = __shfl(lb, s);
                const float srcp = __shfl(rcp, s);
                const int64_t sab = __shfl(ab, s), sbb = __shfl(bb, s);
                // (srb + d) / slb and % slb: srb < slb and d < KRON_CHUNK, so the quotient is at most
                // KRON_CHUNK and the float estimate is off by less than one
                const uint32_t x = srb + (uint32_t)(o - srel);
                uint32_t qq = (uint32_t)((float)x * srcp);
                int64_t rr = (int64_t)x - (int64_t)qq * (int64_t)slb;
                if (rr < 0) {
                    qq--;
                    rr += slb;
                } else if (rr >= (int64_t)slb) {
                    qq++;
                    rr -= slb;
                }
                const int64_t t = p0 + o;
                if (t < nvT) {
                    const int64_t a = sab + qq, b = sbb + rr;
                    kron_store<true, int32_t>(&oci[t], (int32_t)((int64_t)ciA[a] * q + ciB[b]));
                    vop.template put<true>(t, a, b);
                }
            }
        } else {
#pragma unroll 1
            for (int u = 0; u < KRON_WPI; u++) {
                const int64_t t = p0 + u * 64 + lane;
                if (t >= nvT) continue;
                const int64_t R = gb_upper_bound(rpT, rlo, rhi, t) - 1;
                int64_t iA, iB, qa, r0;
                kron_divmod(R, p, &iA, &iB);
                const int64_t b0 = rpB[iB];
                kron_divmod(t - rpT[R], rpB[iB + 1] - b0, &qa, &r0);  // row R holds t: it is not empty
                const int64_t a = rpA[iA] + qa, b = b0 + r0;
                kron_store<true, int32_t>(&oci[t], (int32_t)((int64_t)ciA[a] * q + ciB[b]));
                vop.template put<true>(t, a, b);
            }
        }
    }
}

// kron_method = 1: one thread per output row
template <class V>
__global__ __launch_bounds__(KRON_BLOCK) void k_kron_rows(int64_t nrT, int64_t p, int64_t q,
                                                          const int64_t *__restrict__ rpT,
                                                          const int64_t *__restrict__ rpA,
                                                          const int32_t *__restrict__ ciA,
                                                          const int64_t *__restrict__ rpB,
                                                          const int32_t *__restrict__ ciB,
                                                          int32_t *__restrict__ oci, V vop) {
    for (int64_t R = blockIdx.x * (int64_t)KRON_BLOCK + threadIdx.x; R < nrT; R += (int64_t)gridDim.x * KRON_BLOCK) {
        int64_t iA, iB;
        kron_divmod(R, p, &iA, &iB);
        const int64_t a1 = rpA[iA + 1], b0 = rpB[iB], b1 = rpB[iB + 1];
        int64_t t = rpT[R];
        for (int64_t a = rpA[iA]; a < a1; a++) {
            const int64_t base = (int64_t)ciA[a] * q;
            for (int64_t b = b0; b < b1; b++, t++) {
                oci[t] = (int32_t)(base + ciB[b]);
                vop.template put<false>(t, a, b);
            }
        }
    }
}

}  // namespace

void gb_kronecker(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp op, GB_Obj *A, GB_Obj *B,
                  const gb_desc &d) {
    gb_check_binop(op, false);
    gb_check_binop(accum, true);
    GB_REQUIRE(op->xtype != nullptr, GrB_NOT_IMPLEMENTED, "positional kronecker operator");
    const int xcode = op->xtype->code, zcode = op->ztype->code, opc = op->opcode;
    gb_csr_view av, bv;
    if (d.tran0) gb_get_csc(av, A);
    else gb_get_csr(av, A);
    if (d.tran1) gb_get_csc(bv, B);
    else gb_get_csr(bv, B);
    const int64_t p = bv.nrows, q = bv.ncols;
    int64_t nr = 0, nc = 0, nvT = 0;
    GB_REQUIRE(!__builtin_mul_overflow(av.nrows, p, &nr) && !__builtin_mul_overflow(av.ncols, q, &nc) &&
                   C->nrows == nr && (C->kind == GB_KIND_MATRIX ? C->ncols : 1) == nc,
               GrB_DIMENSION_MISMATCH, "C dimensions do not match kron(A, B)");
    GB_REQUIRE(!__builtin_mul_overflow(av.nvals, bv.nvals, &nvT), GrB_OUT_OF_MEMORY,
               "nvals(A) * nvals(B) overflows");
    // T is iso when the operator reads only iso operands
    const bool use_a = opc != GBAMD_OP_SECOND && opc != GBAMD_OP_PAIR && opc != GBAMD_OP_ANY;
    const bool use_b = opc != GBAMD_OP_FIRST && opc != GBAMD_OP_PAIR;
    const bool t_iso = nvT > 0 && (av.iso || !use_a) && (bv.iso || !use_b);
    const size_t zs = gb_type_size(zcode);
    if (nvT == 0) {
        gb_mat_result T = gb_empty_mat_result(nr, nc, zcode);
        gb_writeback_matrix(C, T, M, d, accum);
        return;
    }
    gb_mat_result T = gb_new_mat_result(nr, nc, zcode, nvT, t_iso);
    gb_scratch s;
    const void *xa = use_a ? gb_view_vals_as(av, xcode, s) : nullptr;
    const void *xb = use_b ? gb_view_vals_as(bv, xcode, s) : nullptr;
    // launches count waves; the knob kron_grid caps the blocks (tests: few blocks, so that a
    // wave runs through many chunks)
    const int wpb = KRON_BLOCK / 64;
    int64_t gcap = gb_knob("kron_grid");
    if (gcap <= 0 || gcap > 8192) gcap = 8192;
    hipLaunchKernelGGL(k_kron_rowptr, dim3(gb_grid((nr + 1 + 63) / 64, wpb, gcap)), dim3(KRON_BLOCK), 0, gb_stream(),
                       nr, p, av.nvals, bv.nvals, av.rowptr, bv.rowptr, T.rowptr);
    GB_LAUNCH_CHECK();
    const bool rows = gb_knob("kron_method") == 1;
    // a wave takes a run of chunks (4 or more, once there are that many)
    const unsigned grid = gb_grid(rows ? (nr + 63) / 64 : ((nvT + KRON_CHUNK - 1) / KRON_CHUNK + 3) / 4, wpb, gcap);
    auto fill = [&](auto vop) {
        using V = decltype(vop);
        if (rows)
            hipLaunchKernelGGL((k_kron_rows<V>), dim3(grid), dim3(KRON_BLOCK), 0, gb_stream(), nr, p, q, T.rowptr,
                               av.rowptr, av.colidx, bv.rowptr, bv.colidx, T.colidx, vop);
        else
            hipLaunchKernelGGL((k_kron_fill<V>), dim3(grid), dim3(KRON_BLOCK), 0, gb_stream(), nvT, nr, p, q,
                               T.rowptr, av.rowptr, av.colidx, bv.rowptr, bv.colidx, T.colidx, vop);
    };
    const bool moves = (opc == GBAMD_OP_FIRST || opc == GBAMD_OP_SECOND || opc == GBAMD_OP_ANY) && xcode == zcode;
    if (t_iso) {
        gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
            using X = decltype(x);
            using Z = decltype(z);
            hipLaunchKernelGGL((k_kron_iso<X, Z>), dim3(1), dim3(1), 0, gb_stream(), opc, (const X *)xa,
                               (const X *)xb, use_a, use_b, (Z *)T.vals);
        });
        fill(kron_move<0>{nullptr, false, nullptr});
    } else if (moves) {
        const bool from_b = opc != GBAMD_OP_FIRST;
        const void *src = from_b ? xb : xa;
        gb_with_size(zs, [&](auto w) { fill(kron_move<(int)sizeof(w)>{src, from_b, T.vals}); });
    } else {
        gb_dispatch_xz(xcode, zcode, [&](auto x, auto z) {
            using X = decltype(x);
            using Z = decltype(z);
            fill(kron_compute<X, Z>{opc, (const X *)xa, (const X *)xb, av.iso, bv.iso, use_a, use_b, (Z *)T.vals});
        });
    }
    GB_LAUNCH_CHECK();
    gb_writeback_matrix(C, T, M, d, accum);
}

extern "C" {

GrB_Info GrB_Matrix_kronecker_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                       const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B,
                                       const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        gb_kronecker(gb_obj_check(C), gb_obj_check(Mask, true), accum, op, gb_obj_check(A), gb_obj_check(B),
                     gb_read_desc(desc));
    });
}

GrB_Info GrB_Matrix_kronecker_Monoid(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                     const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B,
                                     const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_REQUIRE(op, GrB_NULL_POINTER, "monoid is NULL");
        GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid monoid");
        gb_kronecker(gb_obj_check(C), gb_obj_check(Mask, true), accum, op->op, gb_obj_check(A), gb_obj_check(B),
                     gb_read_desc(desc));
    });
}

GrB_Info GrB_Matrix_kronecker_Semiring(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                                       const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B,
                                       const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_REQUIRE(op, GrB_NULL_POINTER, "semiring is NULL");
        GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid semiring");
        gb_kronecker(gb_obj_check(C), gb_obj_check(Mask, true), accum, op->mul, gb_obj_check(A), gb_obj_check(B),
                     gb_read_desc(desc));
    });
}

}  // extern "C"
