// gb_indexop.cuh -- what the builtin index-unary operators compute, shared by GrB_select
// (gb_select.hip: keep the entries whose result is true / non-zero) and GrB_apply with an
// index-unary operator (gb_apply_index.hip: store the result): the device functions of one
// entry (i, j, x) and the host-side casts of the thunk.
#pragma once
#include <algorithm>

#include "gb_dispatch.cuh"

// TRIL .. ROWGT, VALUE*: the result is BOOL; ROWINDEX / COLINDEX / DIAGINDEX: an index
inline bool gb_iop_is_index(int op) { return op >= GBAMD_IOP_ROWINDEX && op <= GBAMD_IOP_DIAGINDEX; }
// the positional operators that look at the row (the others need colidx only)
inline bool gb_iop_needs_row(int op) {
    return op == GBAMD_IOP_TRIL || op == GBAMD_IOP_TRIU || op == GBAMD_IOP_DIAG || op == GBAMD_IOP_OFFDIAG ||
           op == GBAMD_IOP_ROWLE || op == GBAMD_IOP_ROWGT || op == GBAMD_IOP_ROWINDEX || op == GBAMD_IOP_DIAGINDEX;
}

// ROWINDEX i + k, COLINDEX j + k, DIAGINDEX j - i + k, in 64 bits (wrapping); the caller casts to
// the operator's type
GB_DEV int64_t gb_iop_index(int op, int64_t i, int64_t j, int64_t k) {
    const uint64_t base = op == GBAMD_IOP_ROWINDEX ? (uint64_t)i : op == GBAMD_IOP_COLINDEX ? (uint64_t)j
                                                                                            : (uint64_t)j - (uint64_t)i;
    return (int64_t)(base + (uint64_t)k);
}

// the predicate of a positional operator.  An index-valued one keeps z != 0 after the cast to its
// type (the C API's cast of z to bool): zmask holds that type's bits
GB_DEV bool gb_iop_positional(int op, int64_t i, int64_t j, int64_t k, int64_t zmask) {
    switch (op) {
    case GBAMD_IOP_TRIL: return j <= i + k;
    case GBAMD_IOP_TRIU: return j >= i + k;
    case GBAMD_IOP_DIAG: return j == i + k;
    case GBAMD_IOP_OFFDIAG: return j != i + k;
    case GBAMD_IOP_COLLE: return j <= k;
    case GBAMD_IOP_COLGT: return j > k;
    case GBAMD_IOP_ROWLE: return i <= k;
    case GBAMD_IOP_ROWINDEX:
    case GBAMD_IOP_COLINDEX:
    case GBAMD_IOP_DIAGINDEX: return (gb_iop_index(op, i, j, k) & zmask) != 0;
    default: return i > k;  // ROWGT
    }
}

template <class X>
GB_DEV bool gb_iop_value(int op, X x, X y) {
    switch (op) {
    case GBAMD_IOP_VALUEEQ: return x == y;
    case GBAMD_IOP_VALUENE: return x != y;
    case GBAMD_IOP_VALUEGT: return x > y;
    case GBAMD_IOP_VALUEGE: return x >= y;
    case GBAMD_IOP_VALUELT: return x < y;
    default: return x <= y;  // VALUELE
    }
}

// the thunk *y (type ycode) cast to T, the type of code tcode
template <class T>
static T gb_iop_thunk(const void *y, int ycode, int tcode) {
    T out = T();
    gb_cast_scalar(&out, tcode, y, ycode);
    return out;
}

// the thunk of a positional predicate: |k| beyond any index distance decides the same way, and
// the clamp keeps i + k from overflowing
static int64_t gb_iop_thunk_k(const void *y, int ycode) {
    const int64_t lim = (int64_t)1 << 61;
    return std::min(std::max(gb_iop_thunk<int64_t>(y, ycode, GBAMD_T_INT64), -lim), lim);
}

// the thunk of an index-valued operator: cast to the operator's type tcode (INT32 or INT64), then
// widened; *zmask = the bits of that type
static int64_t gb_iop_thunk_index(const void *y, int ycode, int tcode, int64_t *zmask) {
    if (tcode == GBAMD_T_INT32) {
        *zmask = 0xffffffffLL;
        return gb_iop_thunk<int32_t>(y, ycode, GBAMD_T_INT32);
    }
    *zmask = -1;
    return gb_iop_thunk<int64_t>(y, ycode, GBAMD_T_INT64);
}

// the positional thunk of operator opcode whose thunk type is tcode, either kind
static int64_t gb_iop_thunk_pos(int opcode, const void *y, int ycode, int tcode, int64_t *zmask) {
    *zmask = -1;
    return gb_iop_is_index(opcode) ? gb_iop_thunk_index(y, ycode, tcode, zmask) : gb_iop_thunk_k(y, ycode);
}
