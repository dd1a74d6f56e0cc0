// gb_internal.h -- object model and host-side helpers of libgraphblas_amd.so.
//
// One object struct backs GrB_Matrix, GrB_Vector and GrB_Scalar, so the pointer
// casts python-graphblas performs ((GrB_Matrix)v in Vector.inner/outer,
// reference core/vector.py:1643,1686; Vector._as_matrix core/vector.py:186-205;
// Scalar._as_vector core/scalar.py:555-573) are legal: the operation looks at
// the object's kind and converts storage on the fly.
#pragma once
#include <atomic>
#include <utility>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gbamd_codes.h"
#include "gb_state.h"
#include "../../include/graphblas_amd.h"

#define GB_MAGIC 0x6d614d424731ULL   // live object
#define GB_FREED 0x646565724642ULL   // freed object

struct GB_Type_opaque {
    uint64_t magic;
    int code;
    size_t size;
    const char *name;
};
struct GB_BinaryOp_opaque {
    uint64_t magic;
    int opcode;
    GrB_Type xtype, ytype, ztype;  // xtype == nullptr: positional op
    const char *name;
};
struct GB_UnaryOp_opaque {
    uint64_t magic;
    int opcode;
    GrB_Type xtype, ztype;
    const char *name;
};
struct GB_IndexUnaryOp_opaque {
    uint64_t magic;
    int opcode;
    GrB_Type xtype, ytype;  // xtype == nullptr: positional op (thunk INT64)
    const char *name;
};
struct GB_Monoid_opaque {
    uint64_t magic;
    int mcode;
    GrB_Type type;
    GrB_BinaryOp op;
    const char *name;
};
struct GB_Semiring_opaque {
    uint64_t magic;
    GrB_Monoid add;
    GrB_BinaryOp mul;
    const char *name;
    bool user;  // created by GrB_Semiring_new (heap), freed by GrB_Semiring_free
};
struct GB_Descriptor_opaque {
    uint64_t magic;
    int outp, mask, inp0, inp1;
    bool builtin;
    const char *name;
};

struct GB_builtin_entry {
    const char *name;
    int kind;
    void *obj;
};
extern const GB_builtin_entry GB_builtin_registry[];

enum { GB_KIND_MATRIX = 0, GB_KIND_VECTOR = 1, GB_KIND_SCALAR = 2 };

// Per-orientation caches of a matrix, attached lazily by the gb_view_* builders and freed
// together by gb_orient_cache_drop (gb_object.hip), which frees the device pointers and
// resets every field to the defaults below.  Each builder counts its builds (gb_stat_add:
// stat_hub_tables_built, stat_nonempty_built, ...), and every field is named in the READS table
// of tests/derived_state_cases.py next to the probe that reads it after a mutation.
struct gb_orient_cache {
    // hub-chunk table, built by gb_view_hubs (gb_mxv.hip)
    int32_t *hub_tab = nullptr;
    int64_t hub_n = 0, hub_H = 0;
    // bitmap of the non-empty rows, and its per-word exclusive prefix (gb_view_nonempty,
    // gb_mxv.hip): ne_rank[w] = non-empty rows in the words before w, words + 1 entries (the
    // last one their count; row ids are int32, so 32 bits hold it).  Row r's rank among the
    // non-empty rows is ne_rank[r >> 6] + popcount(rows_ne[r >> 6] & bits below r & 63)
    uint64_t *rows_ne = nullptr;
    uint32_t *ne_rank = nullptr;
    // pull heads (gb_view_pullfirst, gb_mxv.hip), one record per non-empty row, indexed by
    // that rank (an empty row is never open in the pull and has no record):
    // 4 int32 -- the row's neighbours with the most entries in the other orientation
    // first, the whole row when it has at most 4 (padding -1), else 3 of them and -2 -- and
    // the row's own length in the other orientation (saturated to 32 bits)
    int32_t *phead = nullptr;
    uint32_t *pdeg = nullptr;
    int64_t maxdeg = -1;  // longest row (host), built with the hub table; -1 unknown
    // long-row chunk table (general SpMV, gb_mxv.hip)
    int32_t *long_tab = nullptr;
    int64_t long_n = 0;
    // hot-column relabel (general SpMV with a dense input, gb_prim.hip gb_view_hot):
    // colidx with the hot_n most frequent columns replaced by INT32_MIN | rank (rank in
    // descending frequency), and the hot columns' original ids in rank order
    int32_t *hot_ci = nullptr;
    int32_t *hot_cols = nullptr;
    int64_t hot_n = 0;
    // narrow copy of the integer values, when every
    // value fits fewer bytes (gb_prim.hip gb_view_narrow): nar_k = 1/2/4 unsigned, -1/-2/-4
    // signed bytes per value, 0 not narrowable; nar_done: computed
    void *nar_vx = nullptr;
    int nar_k = 0;
    bool nar_done = false;
};
void gb_orient_cache_drop(gb_orient_cache &c);

// Device storage.  CSR for matrices; bitmap + dense values for vectors/scalars.
struct GB_Matrix_opaque {
    uint64_t magic;
    int kind;
    GrB_Type type;
    int64_t nrows, ncols;
    bool iso;            // values hold one element that applies to every entry
    // ---- CSR (kind == MATRIX)
    int64_t nvals;       // exact, host-known for CSR
    int64_t *rowptr;     // [nrows+1]
    int32_t *colidx;     // [nvals]
    void *vals;          // [nvals] or [1] when iso
    // cached transpose (CSC), built lazily by gb_csc()
    bool t_valid;
    int64_t *t_rowptr;
    int32_t *t_colidx;
    void *t_vals;
    int64_t *t_perm;     // CSC position -> CSR position of the same entry
    // what the kernels cache about the CSR (0) and the CSC (1) orientation; dropped with the transpose
    gb_orient_cache oc[2];
    // ---- bitmap (kind == VECTOR / SCALAR); length n = nrows (ncols == 1)
    uint64_t *bits;      // [ceil(n/64)]
    void *dense;         // [n] or [1] when iso
    int64_t *d_nvals;    // device counter kept current by every writer
    bool nvals_valid;    // host copy in `nvals` is current
    // host-visible copy of d_nvals published by the kernel that produced it
    // (valid while pub_epoch == gb_epoch(): nothing enqueued since)
    struct gb_host_slot *pub;
    uint64_t pub_seq, pub_epoch;
    // d_nvals[2 .. 2 + GB_HINT_PARTS) hold (in parts) the edge count of this vector's entries in the rows of the
    // push-orientation CSR whose rowptr is hint_key (written by the BFS SpMV that
    // produced it; a stale hint only affects the push/pull choice, never results)
    bool hint_valid;
    const void *hint_key;
    std::string err;
    // ---- column-word bitmap (kind == MATRIX, 1 <= nrows <= 64): the batched-frontier
    // format of gb_colbits.hip.  cw != nullptr: the matrix is held as cw[ncols]
    // presence words (bit r of cw[j] = entry (r, j)) and values cw_vals[j * nrows + r]
    // (or [1] when iso); rowptr/colidx/vals are empty, the count lives in cw_stat[0]
    // (+ the pub mailbox, like a vector's), cw_stat[1] holds the edge hint keyed by
    // hint_key.  Every API entry point outside gb_colbits.hip sees CSR: gb_obj_check
    // converts back (gb_cw_to_csr).
    uint64_t *cw;
    void *cw_vals;
    int64_t *cw_stat;
    // set when a deferred operation on this object failed after its call returned
    // (GrB_INVALID_OBJECT from then on, C API 2.0 nonblocking execution errors)
    GrB_Info invalid = GrB_SUCCESS;
};
typedef GB_Matrix_opaque GB_Obj;

inline GB_Obj *OBJ(const void *p) { return (GB_Obj *)p; }

// ------------------------------------------------------------------ errors
struct gb_exception {
    GrB_Info info;
    std::string msg;
};
[[noreturn]] void gb_throw(GrB_Info info, const std::string &msg);
#define GB_REQUIRE(cond, info, msg) \
    do {                            \
        if (!(cond)) gb_throw(info, msg); \
    } while (0)
void gb_hip_check(hipError_t e, const char *what);
#define GB_HIP(x) gb_hip_check((x), #x)
#define GB_LAUNCH_CHECK() gb_hip_check(hipGetLastError(), "kernel launch")

extern std::atomic<int64_t> g_stat_nvals_copy;
extern std::atomic<int64_t> g_stat_host_push;  // SpMV launches whose push direction the host proved
// named counters of which kernel classes a call used (host-side, off the per-level BFS path):
// GxB_Global_get_int("stat_<name>") reads them; tests assert that a workload reached a class
void gb_stat_add(const char *name, int64_t v);
bool gb_stat_get(const char *name, int64_t *v);
void gb_stat_set(const char *name, int64_t v);  // a counter that holds the last call's figure

// ------------------------------------------------------------------ deferred work (gb_bfs_loop.hip)
// The level-BFS loop's host side defers three things -- a speculatively enqueued next level, a
// pending root (`q[src] = true` on an empty BOOL vector) and a deferred stamp (`v<q> = d`, fused
// into the next SpMV: gb_asg below) -- and no call may observe any of them.  This block is the
// whole contract between that file and the rest of the library.
struct gb_desc;
enum : unsigned { GB_DEFER_SPEC = 1, GB_DEFER_ROOT = 2, GB_DEFER_STAMP = 4, GB_DEFER_ALL = 7 };
extern std::atomic<unsigned> g_deferred;  // a bit per mechanism with something live: 0 outside a BFS loop
// carry out or undo what is live, in the one right order, except the mechanisms in `keep`;
// reader: an object the caller only counts (a speculation stays unless that is its stamp target)
void gb_deferred_resolve(unsigned keep, const void *reader);
// GrB_Vector_setElement_BOOL(v, true, i): true when recorded as the pending root instead
bool gb_root_try_defer(GB_Obj *v, int64_t i);
// w<mask>(:) = x without accum (xc: x as w's type): true when recorded as the deferred stamp;
// a pending root survives the call only as that stamp's mask
bool gb_stamp_try_defer(GB_Obj *w, GB_Obj *mask, const char *xc, const gb_desc &d);
// GrB_Vector_assign_<T>: true when the call is over with *info -- it was the stamp a
// speculation predicted and already carried out (absorbed), or matching it failed
bool gb_deferred_absorb_assign(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const void *x, int xcode,
                               const GrB_Index *I, GrB_Index ni, GrB_Descriptor desc, GrB_Info *info);
// "stat_bfs_spec_adopted" / "stat_bfs_spec_rollbacks" / "stat_deferred_live"
bool gb_deferred_stat(const char *key, int64_t *value);
// GrB_mxv / GrB_vxm (and the row reduction of gb_ops.hip): adopts, fuses or resolves what is live
void gb_do_spmv(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *u, const gb_desc &d,
                bool vxm);
// what that file calls back: the assigns of gb_ops.hip, the one-thread set launch of gb_object.hip
void gb_make_values_writable(GB_Obj *w);
bool gb_assign_all_scalar_fast(GB_Obj *w, GB_Obj *mask, const char *xc, const gb_desc &d);
void gb_vector_assign_scalar(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, const void *x, int xcode,
                             const GrB_Index *I, int64_t ni, const gb_desc &d);
void gb_vec_set_true(GB_Obj *v, int64_t i);

// roctx ranges named by the API entry point around each library call (environment
// GRAPHBLAS_AMD_ROCTX=1; the roctx library is loaded then, never otherwise), so a rocprofv3
// trace with --marker-trace attributes every kernel to the GrB_* / GxB_* call that launched
// it -- the kernel-level counterpart of the reference's Recorder (core/recorder.py:34-178).
extern bool g_roctx_on;
void gb_roctx_push(const char *name);
void gb_roctx_pop();
struct gb_roctx_range {
    bool on;
    explicit gb_roctx_range(const char *name) : on(g_roctx_on && name) {
        if (on) gb_roctx_push(name);
    }
    ~gb_roctx_range() {
        if (on) gb_roctx_pop();
    }
};

// API-boundary wrapper: runs body, converts exceptions to GrB_Info and stores
// the message on the error object (reference core/exceptions.py:124-155 reads
// it back with GrB_<Type>_error on the call's output argument).
// Deferred work other than KEEP's is resolved first (reader: see gb_deferred_resolve); when none
// is live, which is every call outside a BFS loop, that is one load and one branch.
template <unsigned KEEP = 0, class F>
GrB_Info gb_api_impl(GB_Obj *errobj, F &&body, const char *name = nullptr, const void *reader = nullptr) {
    gb_roctx_range range(name);
    try {
        if (KEEP != GB_DEFER_ALL && (g_deferred.load(std::memory_order_acquire) & ~KEEP) != 0)
            gb_deferred_resolve(KEEP, reader);
        body();
        if (errobj && errobj->magic == GB_MAGIC) errobj->err.clear();
        return GrB_SUCCESS;
    } catch (const gb_exception &e) {
        if (errobj && errobj->magic == GB_MAGIC) errobj->err = e.msg;
        return e.info;
    } catch (const std::bad_alloc &) {
        if (errobj && errobj->magic == GB_MAGIC) errobj->err = "out of host memory";
        return GrB_OUT_OF_MEMORY;
    } catch (...) {
        return GrB_PANIC;
    }
}
// the entry point's own name (__func__) names its trace range
#define gb_api(obj, ...) gb_api_impl(obj, __VA_ARGS__, __func__)

// ------------------------------------------------------------------ host-time probes
// Diagnostics of the per-call host path (environment GRAPHBLAS_AMD_HPROF=1): cumulative
// nanoseconds per named section, printed at exit.  A disabled probe costs one load.
extern bool g_hprof_on;
void gb_hprof_add(int slot, const char *name, int64_t ns);
int64_t gb_hprof_now();
struct gb_hprof_scope {
    int slot;
    const char *name;
    int64_t t0;
    gb_hprof_scope(int s, const char *n) : slot(s), name(n), t0(g_hprof_on ? gb_hprof_now() : 0) {}
    ~gb_hprof_scope() {
        if (g_hprof_on) gb_hprof_add(slot, name, gb_hprof_now() - t0);
    }
};
#define GB_HPROF(slot, name) gb_hprof_scope gb_hprof_##slot(slot, name)

// ------------------------------------------------------------------ context
hipStream_t gb_stream();
void gb_require_init();
void gb_sync();
int64_t gb_knob(const char *key);
// persistent zeroed device words (layout: gb_state.h), allocated on first use
unsigned long long *gb_device_state();
// blocks of a launch: ceil(items / per_block) clamped to [1, cap].  A launch that counts waves
// passes per_block = BLOCK / 64.  The caps differ per file and per kernel: they are tuned.
// Test knob "grid_cap" = k > 0 (GxB_Global_set_int) clamps every such grid to k blocks more, so
// that a small shape runs a kernel's later grid sweeps; each call site at which that clamp bit
// is counted as stat_grid_clamped:<file>:<line> ("Grid sweeps").  0: neither.
extern std::atomic<int64_t> g_grid_cap;
void gb_grid_clamped(const char *file, int line);
inline unsigned gb_grid(int64_t items, int64_t per_block, int64_t cap, const char *file = __builtin_FILE(),
                        int line = __builtin_LINE()) {
    int64_t g = (items + per_block - 1) / per_block;
    g = g < 1 ? 1 : g > cap ? cap : g;
    const int64_t k = g_grid_cap.load(std::memory_order_relaxed);
    if (k > 0 && g > k) {
        g = k;
        gb_grid_clamped(file, line);
    }
    return (unsigned)g;
}

// Host-visible mailboxes in pinned coherent memory: a kernel publishes a
// device count with a sequence number (system-scope store); the host spins on
// it instead of a copy + stream synchronisation.
struct gb_host_slot {
    long long seq;
    long long value;
    long long pad[5];  // pad[0]: the column-word kernels' device-written hint (gb_colbits.hip)
    long long host_last;  // host only, never written by a device: the last sequence number issued
};
gb_host_slot *gb_host_slot_alloc();
void gb_host_slot_release(gb_host_slot *s);
gb_host_slot *gb_host_slot_device(gb_host_slot *s);  // device address of the same slot
uint64_t gb_next_pub_seq(gb_host_slot *s);  // the next publish number for slot s
// count of work enqueued through gb_stream() (a published value is current only
// while no later work has been enqueued)
uint64_t gb_epoch();
hipStream_t gb_stream_peek();  // the library stream, without counting an enqueue
// wait for slot->seq == seq; false if the stream drained without it (caller falls back).
// A publisher may instead store one tagged word into seq: bit 63 | (seq & 0x7fffffff) << 32 |
// the 32-bit count (GB_PUB_TAG; a plain seq never has bit 63 set)
#define GB_PUB_TAG (1ULL << 63)
bool gb_host_slot_wait(gb_host_slot *s, uint64_t seq, int64_t *value);
// zero nw bitmap words and (if given) the count, in one launch
void gb_zero_bitmap(uint64_t *bits, int64_t nw, int64_t *d_count);
// count the set bits into *d_count (one launch); publish to the host mailbox when given
void gb_bitmap_count_pub(const uint64_t *bits, int64_t n, int64_t *d_count, gb_host_slot *pub_host, uint64_t seq);  // tuning knobs (0 = auto)

// device memory (stream-ordered pool on the library stream)
void *gb_malloc(size_t bytes);        // throws GrB_OUT_OF_MEMORY
void gb_free(void *p);
template <class T>
T *gb_malloc_n(size_t n) {
    return (T *)gb_malloc(n * sizeof(T));
}
void gb_memset(void *p, int v, size_t bytes);
void gb_copy_d2d(void *dst, const void *src, size_t bytes);
void gb_copy_h2d(void *dst, const void *src, size_t bytes);
void gb_copy_d2h(void *dst, const void *src, size_t bytes);  // synchronises

// scratch owner: frees device buffers at scope exit (stream ordered)
struct gb_scratch {
    void *ptrs[32];
    int n = 0;
    template <class T>
    T *get(size_t count) {
        T *p = gb_malloc_n<T>(count ? count : 1);
        ptrs[n++] = p;
        return p;
    }
    ~gb_scratch() {
        for (int i = 0; i < n; i++) gb_free(ptrs[i]);
    }
};

// ------------------------------------------------------------------ objects
GB_Obj *gb_obj_check(const void *p, bool allow_null = false);      // CSR for matrices
GB_Obj *gb_obj_check_raw(const void *p, bool allow_null = false);  // any internal format
// column-word bitmap matrices (gb_colbits.hip)
void gb_cw_to_csr(GB_Obj *A);    // back to CSR (device work; reads the count)
void gb_cw_release(GB_Obj *A);   // drop the column-word storage without converting
void gb_cw_materialize(GB_Obj *A);  // carry out pending level-stamp layers (values)
GB_Obj *gb_new_object(int kind, GrB_Type type, int64_t nrows, int64_t ncols);
extern "C" void gb_vec_recount(GB_Obj *v);  // a vector's bitmap changed on the device: recount + publish
void gb_obj_free_storage(GB_Obj *A);
void gb_drop_transpose(GB_Obj *A);
int64_t gb_nvals(GB_Obj *A);           // exact (may synchronise for bitmaps)
inline int64_t gb_words(int64_t n) { return (n + 63) >> 6; }
inline bool gb_is_bitmap(const GB_Obj *A) { return A->kind != GB_KIND_MATRIX; }

// Typecast a device array (n elements, or the single iso value).
void gb_cast_array(void *dst, int dst_code, const void *src, int src_code, int64_t n);

// Read-only CSR view of any object (a vector becomes an n x 1 CSR temporary).
struct gb_csr_view {
    int64_t nrows = 0, ncols = 0, nvals = 0;
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    const void *vals = nullptr;
    bool iso = false;
    int tcode = 0;
    // hub chunks (rows longer than hub_H cut into hub_H-edge pieces): pairs (row, piece), then
    // the sections of gb_hub_sections_of (a record per piece, every row's length)
    const int32_t *hubs = nullptr;
    int64_t nhubs = 0, hub_H = 0;
    const uint64_t *nonempty = nullptr;  // bitmap of rows with entries (when attached)
    const uint32_t *ne_rank = nullptr;   // its per-word exclusive prefix, words + 1 entries (attached with it)
    const int32_t *phead = nullptr;      // pull head per non-empty row by rank, 4 int32 (when attached; see gb_orient_cache)
    const uint32_t *pdeg = nullptr;      // row length in the other orientation, by rank (when attached)
    int64_t maxdeg = -1;                 // longest row (host; attached with the hub chunks, -1 unknown)
    const int32_t *lchunks = nullptr;    // long-row chunks (row, piece) of the general SpMV (when attached)
    int64_t nlchunks = -1;
    const void *nvx = nullptr;           // narrow copy of vals (when attached; see gb_orient_cache::nar_vx)
    int nvk = 0;                         // its kind: 1/2/4 unsigned, -1/-2/-4 signed bytes, 0 none
    const int32_t *hcolidx = nullptr;    // hot-column relabelled colidx (when attached; see gb_orient_cache::hot_ci)
    const int32_t *hcols = nullptr;      // the hot columns' original ids, rank order
    int64_t nhot = 0;
    gb_scratch own;
};
void gb_get_csr(gb_csr_view &v, GB_Obj *A);
// The hub table's allocation goes on after its nhubs (row, piece) pairs (and the spare ints
// that follow them) with two sections, built and freed with it: one 16-byte record per piece
// -- its row, its entry count and its first entry position, so the lane that tests a piece
// reads one line and a hit goes to its columns without reading the row's bounds -- and every
// row's length as 32 bits (exact: a row has fewer than 2^31 entries), one read per vertex for
// the next-frontier hint instead of two row pointers.
struct gb_hub_piece {
    int32_t row;  // the piece's row
    int32_t len;  // its entries (hub_H, or fewer for a row's last piece)
    int64_t pos;  // its first entry
};
static_assert(sizeof(gb_hub_piece) == 16, "one 16-byte load per piece");
struct gb_hub_sections {
    const gb_hub_piece *piece = nullptr;  // nhubs records
    const uint32_t *rowlen = nullptr;     // nrows: entries of each row
};
// ints before the records: the pairs and two spare ints, rounded up to 16 bytes
__host__ __device__ inline int64_t gb_hub_prefix_ints(int64_t nhubs) { return (2 * nhubs + 2 + 3) & ~(int64_t)3; }
__host__ __device__ inline gb_hub_sections gb_hub_sections_of(const int32_t *tab, int64_t nhubs) {
    gb_hub_sections s;
    s.piece = reinterpret_cast<const gb_hub_piece *>(tab + gb_hub_prefix_ints(nhubs));
    s.rowlen = reinterpret_cast<const uint32_t *>(s.piece + nhubs);
    return s;
}
inline int64_t gb_hub_table_ints(int64_t nhubs, int64_t nrows) { return gb_hub_prefix_ints(nhubs) + 4 * nhubs + nrows; }
// attach the cached hub-chunk table of matrix A's orientation (0 CSR, 1 CSC) to v
void gb_view_hubs(gb_csr_view &v, GB_Obj *A, int orient, int64_t H);
// attach the cached non-empty-rows bitmap of matrix A's orientation, and its rank prefix, to v
void gb_view_nonempty(gb_csr_view &v, GB_Obj *A, int orient);
// attach the cached pull heads of A's orientation (other_rowptr: the other orientation's row
// pointers, other_n rows) -- the iso pull tests a row's best-connected neighbours first, and
// rows of at most 4 entries without reading their bounds or edges.  The heads are indexed by
// rank among the non-empty rows: v must carry gb_view_nonempty's bitmap and prefix, and gets
// no heads otherwise
void gb_view_pullfirst(gb_csr_view &v, GB_Obj *A, int orient, const int64_t *other_rowptr, int64_t other_n);
void gb_view_long_rows(gb_csr_view &v, GB_Obj *A, int orient);
// attach the cached narrow copy of matrix A's orientation's integer values (built on first use:
// one min/max pass, then a cast) when they fit fewer bytes; v.nvx stays null otherwise
void gb_view_narrow(gb_csr_view &v, GB_Obj *A, int orient);
// attach (building on first use) the hot-column relabel of matrix A's orientation, when the
// matrix is large enough for the x gathers of a dense-input SpMV to miss in L2
void gb_view_hot(gb_csr_view &v, GB_Obj *A, int orient);
// CSC of A (i.e. CSR of A^T), cached on the object when A is a matrix.
void gb_get_csc(gb_csr_view &v, GB_Obj *A);
// the cached CSC of a matrix and, per CSC entry, its CSR position (built on first use)
const int64_t *gb_csc_perm(GB_Obj *A);
// Values of a CSR view cast to type `code` (returns the view's own pointer if same type).
const void *gb_view_vals_as(gb_csr_view &v, int code, gb_scratch &s);

// Read-only bitmap view of any object (an n x 1 matrix becomes a bitmap temporary).
struct gb_bitmap_view {
    int64_t n = 0;
    const uint64_t *bits = nullptr;
    const void *vals = nullptr;
    bool iso = false;
    int tcode = 0;
    const int64_t *count = nullptr;      // device count of entries (nullptr: unknown)
    const long long *mf_hint = nullptr;  // device edge count of the entries (see GB_Obj::hint_key)
    const void *hint_key = nullptr;
    bool full = false;                   // every entry present, known on the host
    int64_t h_nvals = -1;                // entries, when known on the host (-1: not known)
    gb_scratch own;
};
void gb_get_bitmap(gb_bitmap_view &v, GB_Obj *A);
const void *gb_bitmap_vals_as(gb_bitmap_view &v, int code, gb_scratch &s);

// Install freshly computed storage into an object (takes ownership).
void gb_install_csr(GB_Obj *C, int64_t nrows, int64_t ncols, int64_t nvals, int64_t *rowptr,
                    int32_t *colidx, void *vals, bool iso);
void gb_install_bitmap(GB_Obj *C, int64_t n, uint64_t *bits, void *dense, bool iso,
                       int64_t *d_nvals /* may be null: recomputed */);

// bitmap helpers (device work on the library stream)
void gb_bitmap_count(const uint64_t *bits, int64_t n, int64_t *d_count);
void gb_bitmap_to_csr(const uint64_t *bits, const void *dense, bool iso, int64_t n, size_t tsize,
                      int64_t **rowptr, int32_t **colidx, void **vals, int64_t *nvals);
void gb_csr_col_to_bitmap(const gb_csr_view &v, size_t tsize, uint64_t **bits, void **dense,
                          int64_t **d_nvals);

// COO build (sort + duplicate fold) into an empty object; extract tuples to host
void gb_build(GB_Obj *C, const GrB_Index *I, const GrB_Index *J, const void *X, int xcode, bool x_iso,
              int64_t n, GrB_BinaryOp dup);
void gb_extract_tuples(GB_Obj *A, GrB_Index *I, GrB_Index *J, void *X, int xcode, GrB_Index *nvals);
// The device core of the build, shared by gb_build (host arrays) and gb_sparse_io.hip (device
// arrays).  gb_coo_fold: keys (row << 32 | col, bounds-checked) and perm (the identity), n of each,
// are sorted in place and duplicates folded in input order over X_dev (values in `code`; dup_opcode
// < 0 keeps the last): unique keys, folded values and their count come back, caller-owned.
// gb_build_install: such unique sorted tuples (owned from here on) become the storage of the empty
// object C; Xc, the values they were folded from, supplies the iso value under gb_build's dup rule.
void gb_coo_fold(uint64_t *keys, int64_t *perm, const void *X_dev, bool x_iso, int64_t n, int64_t nrows, int code,
                 int dup_opcode, uint64_t **ukeys_out, void **uvals_out, int64_t *nu_out);
bool gb_build_keeps_iso(GrB_BinaryOp dup);  // a one-scalar build stays iso under this dup (NULL: yes)
void gb_build_install(GB_Obj *C, uint64_t *ukeys, void *uvals, int64_t nu, const void *Xc, bool x_iso,
                      GrB_BinaryOp dup);
// the entries of a bitmap vector in index order: dI (nvals indices) and, unless null, dX (nvals
// values in the vector's type), both on the device
void gb_vector_tuples(GB_Obj *A, uint64_t *dI, void *dX);

// expand iso values to a full array of n elements
void *gb_expand_iso(const void *one_value, size_t tsize, int64_t n);

// transpose CSR -> CSR of the transpose (values optional)
// tperm (optional): receives the CSC position -> CSR position map (caller frees)
void gb_transpose_csr(int64_t nrows, int64_t ncols, int64_t nvals, const int64_t *rowptr,
                      const int32_t *colidx, const void *vals, size_t tsize, bool iso,
                      int64_t **trowptr, int32_t **tcolidx, void **tvals, int64_t **tperm = nullptr);

// ------------------------------------------------------------------ index lists
// GrB_ALL, an explicit list, or the GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS encodings
// (gb_extract.hip), expanded on the host and checked against n
struct gb_index_list {
    bool all = false;          // GrB_ALL: idx is empty, the list is 0 .. n-1
    int64_t n = 0;             // length of the list
    std::vector<int64_t> idx;  // explicit indices (all == false)
};
void gb_expand_indices(gb_index_list &L, const GrB_Index *I, GrB_Index ni, int64_t n);
struct gb_mat_result;
struct gb_vec_result;
struct gb_csr_view;
struct gb_bitmap_view;
// the gathers of the extract family (gb_extract.hip), which a subassign (gb_subassign.hip) starts
// with: T = V(I, J); T(k) = V(j, I[k]); T(k) = u(I[k]).  The vector results are counted.
void gb_extract_csr(gb_mat_result &T, const gb_csr_view &v, const gb_index_list &LI, const gb_index_list &LJ);
void gb_extract_line(gb_vec_result &T, const gb_csr_view &v, int64_t j, const gb_index_list &LI);
void gb_extract_vec(gb_vec_result &T, const gb_bitmap_view &uv, const gb_index_list &LI);

// ------------------------------------------------------------------ ops
struct gb_desc {
    bool replace = false, comp = false, structure = false, tran0 = false, tran1 = false;
};
gb_desc gb_read_desc(const GrB_Descriptor d);
inline void gb_check_semiring(GrB_Semiring sr) {
    GB_REQUIRE(sr, GrB_NULL_POINTER, "semiring is NULL");
    GB_REQUIRE(sr->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid semiring");
}
inline void gb_check_binop(GrB_BinaryOp op, bool allow_null) {
    if (!op) {
        GB_REQUIRE(allow_null, GrB_NULL_POINTER, "operator is NULL");
        return;
    }
    GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid operator");
}
inline int64_t gb_ncols_of(const GB_Obj *A) { return A->kind == GB_KIND_MATRIX ? A->ncols : 1; }
// batched-frontier fast paths (gb_colbits.hip): C<M> = A lor.land B with A of at most 64
// rows, and C<M> = x over all indices; false when the call is not of that shape (the
// caller then runs the general path on CSR operands)
bool gb_colbits_mxm(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *B,
                    const gb_desc &d);
bool gb_colbits_assign_scalar(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, const void *x, int xcode,
                              const GrB_Index *I, const GrB_Index *J, const gb_desc &d);

// Effective mask: bitmap of positions where the mask is true (value masks cast
// to bool), for vector outputs; CSR (structure only) for matrix outputs.
struct gb_vmask {
    const uint64_t *bits = nullptr;  // nullptr: no mask
    bool comp = false;
    const int64_t *count = nullptr;  // device count of set mask bits, when known
    int64_t h_count = -1;            // the same count known on the host (-1: not known)
    // value mask of an iso vector, left unmaterialised (only when the caller allows it):
    // the mask is `bits` if the device value *iso_val is nonzero, else empty
    const void *iso_val = nullptr;
    int iso_code = -1;
    gb_scratch own;
};
void gb_make_vmask(gb_vmask &m, GB_Obj *M, const gb_desc &d, int64_t n, bool allow_iso_value = false);

struct gb_mmask {
    bool present = false, comp = false;
    GB_Obj *obj = nullptr;   // the mask matrix when rowptr/colidx are its own CSR (structural)
    gb_csr_view view;        // structure of the mask
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    int64_t nvals = 0;
    gb_scratch own;
};
void gb_make_mmask(gb_mmask &m, GB_Obj *M, const gb_desc &d, int64_t nrows, int64_t ncols);

// Result of a computation before the write-back into C.
struct gb_vec_result {  // bitmap, type code ztype
    int64_t n = 0;
    uint64_t *bits = nullptr;
    void *dense = nullptr;
    bool iso = false;
    int tcode = 0;
    int64_t *d_nvals = nullptr;
    gb_host_slot *pub = nullptr;  // if set, the producing kernel publishes nvals here
    uint64_t pub_seq = 0;
    bool published = false;       // set by the producer when it did publish
    const void *hint_key = nullptr;  // set when d_nvals[2..] hold the edge-count hint parts
};
struct gb_mat_result {  // CSR
    int64_t nrows = 0, ncols = 0, nvals = 0;
    int64_t *rowptr = nullptr;
    int32_t *colidx = nullptr;
    void *vals = nullptr;
    bool iso = false;
    int tcode = 0;
    bool within_mask = false;  // T already restricted to the (non-complemented) mask
};

// C<M,replace> = C accum T  (takes ownership of T's buffers)
// returns true when T was installed into C as is (no merge)
bool gb_writeback_vector(GB_Obj *C, gb_vec_result &T, GB_Obj *M, const gb_desc &d,
                         GrB_BinaryOp accum, bool t_within_mask);
void gb_writeback_matrix(GB_Obj *C, gb_mat_result &T, GB_Obj *M, const gb_desc &d,
                         GrB_BinaryOp accum);

// kernels of the hot path (gb_mxv.hip, gb_spmv_iso.hip, gb_mxm.hip)
// A: rows = output positions (pull); Apush: the other orientation (rows = u's
// positions) or nullptr; the device picks push or pull per call.
// A deferred `w<q>(:) = x` (GrB_Vector_assign with a value or structural mask q,
// no accum / replace, all indices) carried out by the iso SpMV kernel whose input
// is q and whose mask is w's structure (the BFS level loop: v<q> = d;
// q<!v.S> = q lor.land A).  gb_bfs_loop.hip defers such assigns; every other API call
// performs them first (gb_deferred_resolve, called by gb_api).
struct gb_asg {
    uint64_t *bits = nullptr;  // w's bitmap (read as the call's mask, OR q)
    void *vals = nullptr;      // w's dense values
    int size = 0;              // value size in bytes
    unsigned long long x = 0;  // the value's bytes
    const void *q_iso = nullptr;  // q's iso value when q is a value mask (nullptr: structure)
    int q_iso_code = -1;
    int64_t *count = nullptr;  // w's device count
    int64_t h_count = -1;      // w's count before the assign, when the host knew it (-1: not known)
    // u's device count is exact (written by the kernel that produced u, earlier on the stream):
    // an empty u ends the launch early (the speculated level after a BFS's last one)
    bool u_count_exact = false;
    // u is a pending root (gb_bfs_loop.hip): the frontier is {root}; u's storage does not hold it
    int64_t root = -1;
};
void gb_spmv(gb_vec_result &T, const gb_csr_view &A, const gb_csr_view *Apush, gb_bitmap_view &u,
             const gb_vmask &mask, GrB_Semiring sr, bool flip, const gb_asg *asg = nullptr);
bool gb_spmv_result_iso(GrB_Semiring sr, bool a_iso, bool u_iso, bool flip);
// the iso-result (BFS) SpMV (gb_spmv_iso.hip), called by gb_spmv once T is allocated and n > 0;
// av / uv: the operands' values as the multiplier's input type (nullptr: not read)
void gb_spmv_iso(gb_vec_result &T, const gb_csr_view &A, const gb_csr_view *Apush, gb_bitmap_view &u,
                 const gb_vmask &mask, GrB_Semiring sr, bool flip, const gb_asg *asg, const void *av,
                 const void *uv);
#define SPMV_BLOCK 256  // threads per block of the SpMV kernels of both files
#define WAVES_PER_BLOCK (SPMV_BLOCK / 64)
void gb_spgemm(gb_mat_result &T, gb_csr_view &A, gb_csr_view &B, gb_csr_view *BT,
               gb_mmask &mask, GrB_Semiring sr);
// Vector clears without a launch (gb_spmv_iso.hip): a cleared vector takes a pre-zeroed bitmap and
// count from a small pool; its old bitmap is zeroed by the next iso SpMV launch and returns to
// the pool.  Returns false (nothing changed but the old bitmap possibly taken) when the pool
// has nothing of this size: the caller then allocates and zeroes as usual.
bool gb_zpool_clear_vector(GB_Obj *v);

// select (gb_select.hip): T = the entries of A' the index-unary operator keeps for the thunk
// *y (type ycode), written back as C<M> = C accum T
void gb_select(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
               const gb_desc &d);

// apply with an index-unary operator (gb_apply_index.hip): T = f(A'(i, j), i, j, *y) on the structure
// of A' (BOOL for the select operators, the operator's type for ROWINDEX / COLINDEX / DIAGINDEX),
// written back as C<M> = C accum T
void gb_apply_index(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_IndexUnaryOp op, GB_Obj *A, const void *y, int ycode,
                    const gb_desc &d);

// kronecker (gb_kron.hip): T(iA p + iB, jA q + jB) = binop(A'(iA, jA), B'(iB, jB)) for every pair
// of stored entries, written back as C<M> = C accum T
void gb_kronecker(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp binop, GB_Obj *A, GB_Obj *B,
                  const gb_desc &d);

// eWiseUnion (gb_ewise_union.hip): T on A' union B' = add(a, b) / add(a, beta) / add(alpha, b), written
// back as C<M> = C accum T.  alpha and beta point at host values already of add's input type
// (GxB_{Matrix,Vector}_eWiseUnion in gb_scalar_args.cpp read and cast the GrB_Scalars)
void gb_ewise_union(GB_Obj *C, GB_Obj *M, GrB_BinaryOp accum, GrB_BinaryOp add, GB_Obj *A, const void *alpha,
                    GB_Obj *B, const void *beta, const gb_desc &d);
// GxB_Global_get_int asks here first: brings "stat_union_*" up to date after a vector call,
// whose counts stay on the device until somebody reads them
void gb_union_stat_refresh(const char *key);

// concat / split (gb_tile.hip): the entry points are GxB_Matrix_concat / GxB_Matrix_split, which
// leave "stat_concat_bitmap" / "stat_split_bitmap" / "stat_concat_iso" behind (gb_stat_set).
// split builds its tiles around storage it computed: an object of this shape without storage
// (gb_object.hip; the caller installs CSR or a bitmap, or frees it with gb_obj_free_storage)
GB_Obj *gb_new_object_bare(int kind, GrB_Type type, int64_t nrows, int64_t ncols);

// sort (gb_sort.hip): the entry points are GxB_Matrix_sort / GxB_Vector_sort; GxB_Global_get_int
// asks here for "stat_sort_rows_{wave,block,long}" (rows each class took in the last matrix sort,
// read from the device) and for the defaults of "sort_wave_max" / "sort_block_max"
bool gb_sort_stat(const char *key, int64_t *value);
// The sort's row classes at the service of selectk / compactify (gb_selectk.hip): the rows of a
// CSR are ranked ascending by (key, position) and each entry is handed to a trimmed emit.  With
// d the row's length, rank t is entry u = far ? d-1-t : t of the requested order; it is emitted
// when u < m, at slot (reverse ? min(m, d)-1-u : u) of the output row that starts at orp[row].
// keep != nullptr: nothing is moved, keep[input position] = 1 marks the emitted entries, and rows
// of at most m entries are not ranked at all (the caller keeps them whole).
struct gb_rank_job {
    int64_t nrows = 0, nvals = 0;
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    const void *xin = nullptr;  // the values as type xcode: the keys (not read when random)
    int xcode = 0;
    bool random = false;        // key = gb hash of (seed, row, position), 64 bits
    uint64_t seed = 0;
    const void *avals = nullptr;  // the values oC receives, vs bytes each
    int vs = 0;
    int64_t m = 0;
    bool far = false, reverse = false;
    const int64_t *orp = nullptr;
    void *oC = nullptr;       // values (nullptr: not wanted)
    int64_t *oP = nullptr;    // column indices (nullptr: not wanted)
    int32_t *ocol = nullptr;  // the slots: the new column indices (nullptr with keep)
    uint8_t *keep = nullptr;
    int wave_max = 0, block_max = 0;     // 0: the sort's
    unsigned long long *stats = nullptr;  // 4 zeroed device words: rows per class, as the sort's
};
void gb_rank_rows(const gb_rank_job &j);
// The entries of a bitmap in the order of a mode: 0 by index, 1 ascending by (key of xin as
// type xcode, index), 2 ascending by (hash of (seed, 0, position), index).  *idx: n slots, the
// first nvals hold the entries' indices in that order; *off: words + 1 prefix counts, the last
// one nvals.  Both live in s.
void gb_bitmap_order(int64_t n, const uint64_t *bits, const void *xin, int xcode, bool iso, int mode, uint64_t seed,
                     gb_scratch &s, int64_t **idx, int64_t **off);
// the grid of a launch of these two files: gb_grid under the sort's cap, from one call site
unsigned gb_sort_grid(int64_t items, int64_t per_block);

// selectk / compactify (gb_selectk.hip): GxB_Global_get_int asks here for
// "stat_selectk_rows_{all,wave,block,long}" and the defaults of "selectk_wave_max" / "selectk_block_max"
bool gb_selectk_stat(const char *key, int64_t *value);

// scan (gb_scan.hip): the entry points are GxB_Matrix_scan / GxB_Vector_scan; GxB_Global_get_int
// asks here for "stat_scan_rows_{wave,block,long}" (rows of two or more entries each class took in
// the last call) and the defaults of "scan_wave_max" / "scan_block_max" / "scan_chunk"
bool gb_scan_stat(const char *key, int64_t *value);

// hash Gustavson C = A*B (gb_spgemm_hash.hip): flops = per-row product counts
void gb_spgemm_hash(gb_mat_result &T, gb_csr_view &A, gb_csr_view &B, GrB_Semiring sr, bool iso,
                    const void *av, const void *bv, const int64_t *flops);

// scans / sorts (gb_prim.hip)
void gb_exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n);  // out[n] = total
void gb_exclusive_scan_u8(const uint8_t *in, int64_t *out, int64_t n);  // 0/1 flags, int64 prefixes
void gb_exclusive_scan_i32(const int32_t *in, int64_t add_each, int64_t *out, int64_t n);  // of in[i] + add_each
void gb_sort_pairs_u64(uint64_t *keys, int64_t *vals, int64_t n, int end_bit);
void gb_sort_pairs_i32(int32_t *keys, int64_t *vals, int64_t n, int end_bit);
int64_t gb_read_i64(const int64_t *dptr);
// out[e - pbase] = the row of entry e, for the entries of rows [r0, r1): a wave per row, in a
// grid of at most grid_cap blocks (the callers' caps differ)
void gb_rows_of(const int64_t *rowptr, int64_t r0, int64_t r1, int64_t pbase, int64_t *out, int64_t grid_cap);

const char *gb_type_name(int code);
size_t gb_type_size(int code);
GrB_Type gb_type_of(int code);

// ------------------------------------------------------------------ result skeletons
// the buffers of a result of this shape: one value when iso, and no allocation of zero bytes
inline gb_vec_result gb_new_vec_result(int64_t n, int tcode, bool iso) {
    gb_vec_result T;
    T.n = n;
    T.tcode = tcode;
    T.iso = iso;
    T.bits = gb_malloc_n<uint64_t>(gb_words(n) ? gb_words(n) : 1);
    T.dense = gb_malloc((iso || n < 1 ? 1 : n) * gb_type_size(tcode));
    T.d_nvals = gb_malloc_n<int64_t>(1);
    return T;
}
inline gb_mat_result gb_new_mat_result(int64_t nrows, int64_t ncols, int tcode, int64_t nvals, bool iso) {
    gb_mat_result T;
    T.nrows = nrows;
    T.ncols = ncols;
    T.tcode = tcode;
    T.nvals = nvals;
    T.iso = iso;
    T.rowptr = gb_malloc_n<int64_t>(nrows + 1);
    T.colidx = gb_malloc_n<int32_t>(nvals < 1 ? 1 : nvals);
    T.vals = gb_malloc((iso || nvals < 1 ? 1 : nvals) * gb_type_size(tcode));
    return T;
}
// the matrix result of this shape without entries (no call site builds an empty vector result)
inline gb_mat_result gb_empty_mat_result(int64_t nrows, int64_t ncols, int tcode) {
    gb_mat_result T = gb_new_mat_result(nrows, ncols, tcode, 0, false);
    gb_memset(T.rowptr, 0, (nrows + 1) * sizeof(int64_t));
    return T;
}
