// gb_bfs_loop.hip -- the host side of the level-BFS loop: everything the library defers so that
// the notebook loop (reference notebooks/Example B.1 -- Level BFS.ipynb cell 8)
//     q[src] = True
//     v[:](mask=q.V) << d ;  q(~v.S, replace) << q.vxm(A) ;  if q.nvals == 0: break ;  d += 1
// runs back to back on the GPU, and GrB_mxv / GrB_vxm, whose call (gb_do_spmv) drives all of it:
//   the pending root   q[src] = True on an empty BOOL vector is recorded, not launched; the first
//                      level's kernel pushes from src (gb_spmv_iso.hip gb_push_root)
//   the deferred stamp v<q> = d is recorded and carried out inside the next SpMV's kernel (gb_asg)
//   level speculation  the level after the one just issued is enqueued before the host asks for
//                      it, then adopted or rolled back
// The promise: no call ever observes a deferred state.  Every API call tests g_deferred (one load,
// gb_api_impl) and has gb_deferred_resolve carry out or undo what is live, except the calls that
// continue the loop, which name what they keep: the stamp keeps a pending root, a count of
// anything but v keeps a speculation, the SpMV resolves all three itself.  The block "deferred
// work" in gb_internal.h is the whole interface; the kernels are in gb_spmv_iso.hip.
//
// Locks.  g_spec_mu is the outer lock; g_pend_mu and g_root_mu (and the mutex inside
// true_dev) are leaves, taken one at a time, never one inside another.  The only nesting
// is under g_spec_mu: the rollback (spec_rollback_locked) re-issues an absorbed stamp through
// gb_vector_assign_scalar, which takes g_root_mu (root_pending, root_flush) and then g_pend_mu
// (gb_stamp_try_defer), each released before the next -- and clears the speculation's record and
// bit first, so that nothing it calls comes back for g_spec_mu.  gb_deferred_resolve takes the
// three in that order, one after the other.  Nothing that runs under g_pend_mu (the flushed
// assign's launch) or g_root_mu (the set launch) reaches any of the three mechanisms.
#include <algorithm>
#include <atomic>
#include <mutex>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

std::atomic<unsigned> g_deferred{0};
static bool live(unsigned bit) { return (g_deferred.load(std::memory_order_acquire) & bit) != 0; }
static void mark(unsigned bit, bool on) {
    if (on) g_deferred.fetch_or(bit, std::memory_order_release);
    else g_deferred.fetch_and(~bit, std::memory_order_release);
}

// ================================================================== the pending root
// `GrB_Vector_setElement_BOOL(q, true, i)` on an empty BOOL vector -- the BFS start -- is recorded
// instead of launched; the level SpMV of the notebook shape that reads q consumes it (root_take),
// the deferred stamp `v<q> = 1` before it keeps it pending, and any other call materialises it
// first (root_flush: the single-thread set launch it replaced).  Knob root_defer = 1 disables it.
static std::mutex g_root_mu;
static GB_Obj *g_root_v = nullptr;
static int64_t g_root_i = -1;

static void root_flush() {
    std::lock_guard<std::mutex> lk(g_root_mu);
    GB_Obj *v = g_root_v;
    g_root_v = nullptr;
    mark(GB_DEFER_ROOT, false);
    if (!v || v->magic != GB_MAGIC) return;
    gb_vec_set_true(v, g_root_i);
}
static bool root_pending(const GB_Obj *v) {
    if (!live(GB_DEFER_ROOT)) return false;
    std::lock_guard<std::mutex> lk(g_root_mu);
    return v && v == g_root_v;
}
// the root index, the record cleared; -1 when v holds none
static int64_t root_take(GB_Obj *v) {
    std::lock_guard<std::mutex> lk(g_root_mu);
    if (!v || v != g_root_v) return -1;
    g_root_v = nullptr;
    mark(GB_DEFER_ROOT, false);
    return g_root_i;
}
// one device byte holding true (a consumed root's iso value)
static const void *true_dev() {
    static std::mutex mu;
    static bool *p = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!p) {
        GB_HIP(hipMalloc((void **)&p, 16));
        const unsigned char one[16] = {1};
        GB_HIP(hipMemcpy(p, one, sizeof(one), hipMemcpyHostToDevice));
    }
    return p;
}

bool gb_root_try_defer(GB_Obj *v, int64_t i) {
    if (v->kind != GB_KIND_VECTOR || v->type->code != GBAMD_T_BOOL || !v->nvals_valid || v->nvals != 0 || v->dense ||
        !v->bits || v->invalid != GrB_SUCCESS || gb_knob("root_defer") == 1)
        return false;
    if (live(GB_DEFER_ROOT)) root_flush();  // one record at a time
    v->dense = gb_malloc(sizeof(bool));     // written when the root materialises (or never read)
    v->iso = true;
    v->nvals = 1;  // known on the host
    v->hint_valid = false;
    std::lock_guard<std::mutex> lk(g_root_mu);
    g_root_v = v;
    g_root_i = i;
    mark(GB_DEFER_ROOT, true);
    return true;
}

// ================================================================== the deferred stamp
// `w<q>(:) = x` (gb_asg) is recorded instead of launched; the next GrB_mxv / GrB_vxm whose input
// is q and whose mask is w's structure performs it inside its kernel; any other call performs it
// first (stamp_flush).  Knob fuse_assign = 1 disables it.
static std::mutex g_pend_mu;
static struct {
    GB_Obj *w = nullptr, *mask = nullptr;
    char x[16];
    gb_desc d;
    int64_t w_count = -1;  // w's count before the deferral, when the host knew it
} g_pend;

// A failure of the deferred assign is an execution error of `w`, not of the call that
// triggered the flush: it is recorded on w (message + GrB_INVALID_OBJECT from then on,
// as the C API 2.0 prescribes for nonblocking execution errors) and the triggering call
// goes on.  The pending record is cleared only once the assign has been issued or has
// failed and been recorded.  (Its mask may be a pending root: the caller flushes that first.)
static void stamp_flush() {
    std::lock_guard<std::mutex> lk(g_pend_mu);
    GB_Obj *w = g_pend.w, *m = g_pend.mask;
    if (w && w->magic == GB_MAGIC && m && m->magic == GB_MAGIC && w->invalid == GrB_SUCCESS) {
        try {
            // fault injection for the tests (knob inject_flush_fail = 1)
            GB_REQUIRE(gb_knob("inject_flush_fail") != 1, GrB_OUT_OF_MEMORY, "injected failure");
            gb_assign_all_scalar_fast(w, m, g_pend.x, g_pend.d);
        } catch (const gb_exception &e) {
            w->invalid = e.info;
            w->err = "deferred GrB_Vector_assign failed: " + e.msg;
        } catch (const std::bad_alloc &) {
            w->invalid = GrB_OUT_OF_MEMORY;
            w->err = "deferred GrB_Vector_assign failed: out of host memory";
        }
    }
    g_pend.w = g_pend.mask = nullptr;
    mark(GB_DEFER_STAMP, false);
}

bool gb_stamp_try_defer(GB_Obj *w, GB_Obj *mask, const char *xc, const gb_desc &d) {
    // a pending root stays pending only under the deferred stamp whose mask it is
    if (live(GB_DEFER_ROOT) && !(mask && root_pending(mask) && !root_pending(w))) root_flush();
    if (gb_knob("fuse_assign") == 1) return false;
    if (!mask || mask == w || w->kind == GB_KIND_MATRIX || mask->kind == GB_KIND_MATRIX) return false;
    if (d.comp || d.replace || w->type->size > 8 || mask->nrows != w->nrows || !w->bits) return false;
    if (!d.structure && !(mask->iso && mask->dense)) return false;  // per-entry values: assign now
    gb_make_values_writable(w);
    std::lock_guard<std::mutex> lk(g_pend_mu);
    g_pend.w = w;
    g_pend.mask = mask;
    memcpy(g_pend.x, xc, sizeof(g_pend.x));
    g_pend.d = d;
    g_pend.w_count = w->nvals_valid ? w->nvals : -1;
    mark(GB_DEFER_STAMP, true);
    w->nvals_valid = false;
    w->hint_valid = false;
    return true;
}

// take the pending assign into `asg` when this SpMV can carry it out (see above)
static bool take_pending_assign(gb_asg &asg, GB_Obj *w, GB_Obj *mask, GB_Obj *A, GB_Obj *u, const gb_desc &d,
                                bool iso_result) {
    std::lock_guard<std::mutex> lk(g_pend_mu);
    GB_Obj *pw = g_pend.w;
    if (!pw || pw != mask || g_pend.mask != u || !d.structure || w == pw || A == pw || !iso_result ||
        u->kind == GB_KIND_MATRIX || pw->nrows != u->nrows)
        return false;
    asg.bits = pw->bits;
    asg.vals = pw->dense;
    asg.size = (int)pw->type->size;
    memcpy(&asg.x, g_pend.x, sizeof(asg.x));
    asg.q_iso = g_pend.d.structure ? nullptr : u->dense;
    asg.q_iso_code = u->type->code;
    asg.count = pw->d_nvals;
    asg.h_count = g_pend.w_count;
    g_pend.w = g_pend.mask = nullptr;
    mark(GB_DEFER_STAMP, false);
    return true;
}

// ================================================================== the operand views of one SpMV
// A' along the pulled rows (+ the other orientation for the push direction of iso results), u's
// bitmap (+ its next-frontier edge hint), the mask.
struct spmv_views {
    gb_csr_view av, pv;
    const gb_csr_view *push = nullptr;
    gb_bitmap_view uv;
    gb_vmask m;
    bool iso_result = false;
};

static void spmv_build_views(spmv_views &V, GB_Obj *mask, GrB_Semiring sr, GB_Obj *A, GB_Obj *u, const gb_desc &d,
                             bool vxm, int64_t a_rows, const gb_asg *asg) {
    const bool use_csc = vxm ? !d.tran1 : d.tran0;
    if (use_csc) gb_get_csc(V.av, A);
    else gb_get_csr(V.av, A);
    gb_view_nonempty(V.av, A, use_csc ? 1 : 0);
    gb_get_bitmap(V.uv, u);
    if (u->kind != GB_KIND_MATRIX && u->hint_valid) {
        V.uv.mf_hint = (const long long *)(u->d_nvals + 2);  // GB_HINT_PARTS parts
        V.uv.hint_key = u->hint_key;
    }
    if (u->kind != GB_KIND_MATRIX && u->nvals_valid) V.uv.h_nvals = u->nvals;
    gb_make_vmask(V.m, mask, d, a_rows);
    // an empty mask vector: its count is known on the host (value or structure alike)
    if (V.m.bits && mask && mask->kind != GB_KIND_MATRIX && mask->nvals_valid && mask->nvals == 0) V.m.h_count = 0;
    // the fused assign's target is the mask (take_pending_assign): its count before this call's
    // assign, as the host knew it when the assign was deferred (a BFS's first level after
    // clearing v: 0), lets gb_spmv_iso pick push on the host without the prep launch
    // -- a stored-entry count equals the set-bit count only for a structural mask; for a value
    // mask it is an upper bound, which still bounds the open rows of a complemented mask from
    // below but says nothing for a plain one
    if (asg && V.m.bits && V.m.h_count < 0 && asg->h_count >= 0 && (d.structure || d.comp))
        V.m.h_count = asg->h_count;
    // the other orientation (cached on matrices) enables the push direction for iso results
    V.iso_result = gb_spmv_result_iso(sr, A->iso, V.uv.iso, vxm);
    if (!V.iso_result) gb_view_long_rows(V.av, A, use_csc ? 1 : 0);
    V.uv.full = u->kind != GB_KIND_MATRIX && u->nvals_valid && u->nvals == u->nrows && u->nrows > 0;
    if (!V.iso_result && V.uv.full && !V.uv.iso && A->kind == GB_KIND_MATRIX && !gb_sr_describe(sr).positional)
        gb_view_hot(V.av, A, use_csc ? 1 : 0);
    // (pull only, spmv_direction 1: no push, but the pull keeps its heads -- the pull it forces is
    // the default's pull, packed rows included)
    if (A->kind == GB_KIND_MATRIX && V.iso_result) {
        if (use_csc) gb_get_csr(V.pv, A);
        else gb_get_csc(V.pv, A);
        if (gb_knob("spmv_direction") != 1) {
            int64_t H = gb_knob("push_heavy");
            gb_view_hubs(V.pv, A, use_csc ? 0 : 1, H > 0 ? H : 512);
            V.push = &V.pv;
        }
        if (gb_knob("pull_first") != 1) gb_view_pullfirst(V.av, A, use_csc ? 1 : 0, V.pv.rowptr, V.pv.nrows);
    }
}

// ================================================================== level speculation
// (knob bfs_spec = 1 disables).  Each level's launch waits on the host: the previous level's
// count reaches the host's nvals, then the host issues the next assign and vxm (≈ 12 µs of idle
// GPU per level, measured with rocprofv3 kernel traces).  After a level of exactly
// the loop's shape (the deferred stamp `v<q> = x` fused into `q<!v.S, replace> = q (+).(x) A`,
// integer x), the next level -- stamp x + 1, then the same SpMV on the q just produced -- is
// enqueued right behind it, into a result of its own with a mailbox of its own.  When the host
// then issues exactly that assign and that vxm, the assign is absorbed and the vxm installs the
// speculative result (and enqueues the level after it): the GPU runs the levels back to back.
// Anything else -- another call touching v, q or A, a different stamp value, descriptor or
// semiring -- rolls the speculation back first: the speculative stamp only added q's bits to v (q
// and v are disjoint: q was produced under the mask !v.S), so clearing q's bits in v and
// subtracting q's count restores v exactly (nothing to undo when q is empty, the loop's normal
// exit), the speculative result is dropped, and an absorbed assign is re-issued.  Reads that the
// speculation leaves alone (nvals of any object but v) go through.
static std::atomic<int64_t> g_stat_adopted{0}, g_stat_rollbacks{0};
static std::mutex g_spec_mu;
static struct {
    bool active = false;
    GB_Obj *q = nullptr, *v = nullptr, *A = nullptr;  // w == u == q, mask == the stamp's target v
    GrB_Semiring sr = nullptr;
    gb_desc d;                     // the SpMV's descriptor
    bool vxm = false;
    bool stamp_struct = false;     // the stamp's mask: q.S (true) or q's value (iso q)
    unsigned long long x = 0;      // the predicted stamp value (v's type, its bytes)
    gb_vec_result T;               // the speculative next q
    gb_host_slot *slot = nullptr;  // its mailbox (swapped with q's on adoption)
    uint64_t *q_bits = nullptr;    // the q the speculative kernel read (and stamped into v)
    int64_t *q_dn = nullptr;
    const void *q_iso = nullptr;   // its iso value (a value-mask stamp happens only when nonzero)
    int q_iso_code = 0;
    bool assign_matched = false;   // the host has issued the predicted stamp (absorbed)
} g_spec;

bool gb_deferred_stat(const char *key, int64_t *value) {
    if (!strcmp(key, "stat_deferred_live")) {  // read without resolving: what the next call will meet
        *value = (int64_t)g_deferred.load(std::memory_order_acquire);
        return true;
    }
    const bool adopted = !strcmp(key, "stat_bfs_spec_adopted");
    if (!adopted && strcmp(key, "stat_bfs_spec_rollbacks")) return false;
    *value = (adopted ? g_stat_adopted : g_stat_rollbacks).load(std::memory_order_relaxed);
    return true;
}

// q_iso: q's iso value when the stamp's mask was q's values (nullptr: q.S) -- an iso-false q
// stamped nothing, so there is nothing to take back
__global__ void k_spec_unstamp(int64_t nw, uint64_t *__restrict__ vbits, const uint64_t *__restrict__ qbits,
                               int64_t *__restrict__ vcount, const int64_t *__restrict__ qcount, const void *q_iso,
                               int q_iso_code) {
    if (q_iso && !gb_dyn_nonzero(q_iso, q_iso_code)) return;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nw; k += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t qb = qbits[k];
        if (qb) vbits[k] &= ~qb;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) vcount[0] -= qcount[0];
}

static bool spec_int_type(int code) { return code >= GBAMD_T_INT8 && code <= GBAMD_T_UINT64; }

static unsigned long long spec_next(unsigned long long x, size_t size) {
    const unsigned long long m = size >= 8 ? ~0ULL : ((1ULL << (8 * size)) - 1);
    return (x + 1) & m;  // two's complement wrap in v's width
}

static void spec_drop_result() {
    gb_free(g_spec.T.bits);
    gb_free(g_spec.T.dense);
    gb_free(g_spec.T.d_nvals);
    g_spec.T = gb_vec_result{};
}

// undo the speculative level (g_spec_mu held); see above.  Never throws: the rollback runs on
// behalf of whichever call found the speculation in its way, so a failure of the unstamp or of
// the re-issued absorbed stamp is an execution error of v -- recorded on v (GrB_INVALID_OBJECT
// from then on, like a failed deferred assign in stamp_flush), not of the calling API.
static void spec_rollback_locked() {
    if (!g_spec.active) return;
    GB_Obj *q = g_spec.q, *v = g_spec.v;
    g_spec.active = false;
    mark(GB_DEFER_SPEC, false);
    g_stat_rollbacks.fetch_add(1, std::memory_order_relaxed);
    const bool matched = g_spec.assign_matched;
    g_spec.assign_matched = false;
    auto record = [&](GrB_Info info, const std::string &msg) {
        if (v->magic != GB_MAGIC) return;
        v->invalid = info;
        v->err = "speculative BFS level rollback failed: " + msg;
    };
    try {
        const bool q_empty = q->nvals_valid && q->nvals == 0 && q->bits == g_spec.q_bits;
        if (!q_empty) {
            const int64_t nw = gb_words(v->nrows);
            const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((nw + 255) / 256, 1), 1024);
            hipLaunchKernelGGL(k_spec_unstamp, dim3(grid), dim3(256), 0, gb_stream(), nw, v->bits, g_spec.q_bits,
                               v->d_nvals, g_spec.q_dn, g_spec.stamp_struct ? nullptr : g_spec.q_iso,
                               g_spec.q_iso_code);
            GB_LAUNCH_CHECK();
        }
        v->nvals_valid = false;
        v->hint_valid = false;
        if (matched) {
            // the host issued the predicted stamp; it was absorbed: issue it now -- the record and
            // its bit are already cleared, so this takes only the leaf locks (see the top)
            // (fault injection for the tests: knob inject_spec_fail = 1)
            GB_REQUIRE(gb_knob("inject_spec_fail") != 1, GrB_OUT_OF_MEMORY, "injected failure");
            gb_desc ad;
            ad.structure = g_spec.stamp_struct;
            char xc[16] = {0};
            memcpy(xc, &g_spec.x, sizeof(g_spec.x));
            gb_vector_assign_scalar(v, q, nullptr, xc, v->type->code, GrB_ALL, v->nrows, ad);
        }
    } catch (const gb_exception &e) {
        record(e.info, e.msg);
    } catch (const std::bad_alloc &) {
        record(GrB_OUT_OF_MEMORY, "out of host memory");
    } catch (...) {
        record(GrB_PANIC, "unknown error");
    }
    try {
        spec_drop_result();
    } catch (...) {
        // freeing goes back to the caching allocator; nothing to record
    }
}

// the one place that knows the order: the speculation first (its rollback may re-issue, and so
// defer again, a stamp), then the root (the stamp reads it: flushing the stamp overrides keeping
// the root), then the stamp.  keep: GB_DEFER_* bits left as they are; reader: an object the
// caller only counts -- a speculation stays unless reader is its stamp target.
void gb_deferred_resolve(unsigned keep, const void *reader) {
    if (!(keep & GB_DEFER_SPEC) && live(GB_DEFER_SPEC)) {
        std::lock_guard<std::mutex> lk(g_spec_mu);
        if (g_spec.active && (!reader || OBJ(reader) == g_spec.v)) spec_rollback_locked();
    }
    const bool stamp = !(keep & GB_DEFER_STAMP) && live(GB_DEFER_STAMP);
    if ((stamp || !(keep & GB_DEFER_ROOT)) && live(GB_DEFER_ROOT)) root_flush();
    if (stamp) stamp_flush();
}

// enqueue the level after the one just issued (g_spec_mu held): stamp v<q> = x, then
// q' = q (+).(x) A under !v.S into a result of its own
static void spec_launch_locked(GB_Obj *q, GB_Obj *v, GB_Obj *A, GrB_Semiring sr, const gb_desc &d, bool vxm,
                               unsigned long long x, bool stamp_struct) {
    gb_asg asg;
    asg.bits = v->bits;
    asg.vals = v->dense;
    asg.size = (int)v->type->size;
    asg.x = x;
    asg.q_iso = stamp_struct ? nullptr : q->dense;
    asg.q_iso_code = q->type->code;
    asg.count = v->d_nvals;
    asg.h_count = -1;
    asg.u_count_exact = true;  // q was just produced by the kernel before this one
    spmv_views V;
    spmv_build_views(V, v, sr, A, q, d, vxm, q->nrows, &asg);
    if (!V.iso_result) return;
    if (!g_spec.slot) g_spec.slot = gb_host_slot_alloc();
    gb_vec_result T;
    T.pub = g_spec.slot;
    T.pub_seq = gb_next_pub_seq(T.pub);
    gb_spmv(T, V.av, V.push, V.uv, V.m, sr, vxm, &asg);
    g_spec.T = T;
    g_spec.q = q;
    g_spec.v = v;
    g_spec.A = A;
    g_spec.sr = sr;
    g_spec.d = d;
    g_spec.vxm = vxm;
    g_spec.stamp_struct = stamp_struct;
    g_spec.x = x;
    g_spec.q_bits = q->bits;
    g_spec.q_dn = q->d_nvals;
    g_spec.q_iso = q->dense;
    g_spec.q_iso_code = q->type->code;
    g_spec.assign_matched = false;
    g_spec.active = true;
    mark(GB_DEFER_SPEC, true);
}

static bool same_desc(const gb_desc &a, const gb_desc &b) {
    return a.replace == b.replace && a.comp == b.comp && a.structure == b.structure && a.tran0 == b.tran0 &&
           a.tran1 == b.tran1;
}

// after a level whose stamp was fused (gb_do_spmv): speculate the next one when the call has the
// notebook loop's shape
static void spec_after_level(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *u,
                             const gb_desc &d, bool vxm, const gb_asg &asg, bool direct, bool published) {
    if (gb_knob("bfs_spec") == 1 || (gb_knob("iso_dbg") & ~(128 | 512)) != 0) return;  // 128, 512: A/B orders, exact
    if (!direct || !published || accum || w != u || !mask || !d.replace || !d.comp || !d.structure) return;
    if (w->kind == GB_KIND_MATRIX || mask->kind == GB_KIND_MATRIX || A->kind != GB_KIND_MATRIX || A->cw) return;
    if (!spec_int_type(mask->type->code) || asg.bits != mask->bits || asg.vals != mask->dense) return;
    std::lock_guard<std::mutex> lk(g_spec_mu);
    if (g_spec.active) spec_rollback_locked();  // cannot happen (gb_do_spmv adopted or rolled back)
    try {
        spec_launch_locked(w, mask, A, sr, d, vxm, spec_next(asg.x, mask->type->size), asg.q_iso == nullptr);
    } catch (...) {
        // a speculation that could not be set up is simply not made (the level itself is done);
        // if its kernel did run, undo it like any other
        if (g_spec.active) spec_rollback_locked();
        return;
    }
    // the level's own count stays readable from its mailbox: the speculative launch does not touch w
    if (w->pub_seq) w->pub_epoch = gb_epoch();
}

// the host issues `w<mask> = x` (all indices, no accum): absorbed when it is the predicted stamp
// Absorbs only what the normal path would carry out without error: GrB_ALL with ni == n, a
// valid (not execution-failed) target and mask; anything else rolls back and takes gb_api.
static bool spec_match_assign(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, const void *x, int xcode,
                              const GrB_Index *I, int64_t ni, GrB_Descriptor desc) {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    if (!g_spec.active) return false;
    bool ok = !g_spec.assign_matched && w == g_spec.v && mask == g_spec.q && !accum && I == GrB_ALL &&
              !live(GB_DEFER_STAMP) && w->magic == GB_MAGIC && ni == w->nrows && w->invalid == GrB_SUCCESS && mask &&
              mask->magic == GB_MAGIC && mask->invalid == GrB_SUCCESS;
    if (ok) {
        gb_desc ad;
        try {
            ad = gb_read_desc(desc);
        } catch (...) {
            ok = false;
        }
        ok = ok && !ad.replace && !ad.comp && ad.structure == g_spec.stamp_struct && !ad.tran0 && !ad.tran1;
    }
    if (ok) {
        unsigned long long xv = 0;
        gb_cast_scalar(&xv, w->type->code, x, xcode);
        ok = xv == g_spec.x;
    }
    if (!ok) {
        spec_rollback_locked();
        return false;
    }
    g_spec.assign_matched = true;
    w->err.clear();
    w->nvals_valid = false;
    w->hint_valid = false;
    return true;
}

// The match runs inside the API wrapper so that nothing it raises crosses the C boundary.  True:
// the call is over, *info is its result (absorbed, or the match failed); false: not absorbed,
// the speculation (if any) rolled back -- the caller carries the assign out.
bool gb_deferred_absorb_assign(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const void *x, int xcode,
                               const GrB_Index *I, GrB_Index ni, GrB_Descriptor desc, GrB_Info *info) {
    if (!live(GB_DEFER_SPEC) || !w || OBJ(w)->magic != GB_MAGIC) return false;
    bool absorbed = false;
    *info = gb_api_impl<GB_DEFER_ALL>(OBJ(w), [&] {
        absorbed = spec_match_assign(OBJ(w), mask ? OBJ(mask) : nullptr, accum, x, xcode, I, (int64_t)ni, desc);
    });
    return absorbed || *info != GrB_SUCCESS;
}

// the host issues the predicted SpMV: install the speculative result and speculate again
static bool spec_try_adopt(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *u,
                           const gb_desc &d, bool vxm) {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    if (!g_spec.active) return false;
    const bool ok = g_spec.assign_matched && w == g_spec.q && u == g_spec.q && mask == g_spec.v && A == g_spec.A &&
                    sr == g_spec.sr && !accum && vxm == g_spec.vxm && same_desc(d, g_spec.d) &&
                    w->bits == g_spec.q_bits && g_spec.T.published && gb_knob("bfs_spec") != 1 &&
                    !live(GB_DEFER_STAMP);
    if (!ok) {
        spec_rollback_locked();
        return false;
    }
    GB_Obj *q = w, *v = mask;
    gb_vec_result T = g_spec.T;
    g_spec.T = gb_vec_result{};
    g_spec.active = false;
    mark(GB_DEFER_SPEC, false);
    g_stat_adopted.fetch_add(1, std::memory_order_relaxed);
    std::swap(q->pub, g_spec.slot);  // the result's mailbox becomes q's; q's old one, the next speculation's
    const void *hk = T.hint_key;
    const uint64_t seq = T.pub_seq;
    gb_writeback_vector(q, T, v, d, nullptr, true);  // replace, T within the mask: installed as is
    q->pub_seq = seq;
    q->hint_valid = hk != nullptr;
    q->hint_key = hk;
    v->nvals_valid = false;
    v->hint_valid = false;
    try {
        spec_launch_locked(q, v, A, sr, d, vxm, spec_next(g_spec.x, v->type->size), g_spec.stamp_struct);
    } catch (...) {
        if (g_spec.active) spec_rollback_locked();
    }
    q->pub_epoch = gb_epoch();
    return true;
}

// ================================================================== mxv / vxm
void gb_do_spmv(GB_Obj *w, GB_Obj *mask, GrB_BinaryOp accum, GrB_Semiring sr, GB_Obj *A, GB_Obj *u, const gb_desc &d,
                bool vxm) {
    GB_HPROF(1, "do_spmv total");
    gb_check_semiring(sr);
    gb_check_binop(accum, true);
    // rows of the operand matrix the kernel pulls along:
    //   mxv:  w = A' u    -> rows of A'          (A' = A: CSR, A' = A^T: CSC)
    //   vxm:  w = u' A'   -> rows of A'^T        (A' = A: CSC, A' = A^T: CSR)
    int64_t a_rows = (vxm ? (d.tran1 ? A->nrows : gb_ncols_of(A)) : (d.tran0 ? gb_ncols_of(A) : A->nrows));
    int64_t a_cols = (vxm ? (d.tran1 ? gb_ncols_of(A) : A->nrows) : (d.tran0 ? A->nrows : gb_ncols_of(A)));
    GB_REQUIRE(u->nrows == a_cols && gb_ncols_of(u) == 1, GrB_DIMENSION_MISMATCH, "u size does not match A");
    GB_REQUIRE(w->nrows == a_rows && gb_ncols_of(w) == 1, GrB_DIMENSION_MISMATCH, "w size does not match A");
    // the next BFS level, launched speculatively by the previous call (below): adopted when this
    // call is the one predicted, rolled back otherwise
    if (live(GB_DEFER_SPEC) && spec_try_adopt(w, mask, accum, sr, A, u, d, vxm)) return;
    // a deferred `mask<u> = x` (the BFS level stamp) is fused into this call's kernel, or done now
    gb_asg asg;
    bool fused = false;
    if (live(GB_DEFER_STAMP)) {
        fused = A->kind == GB_KIND_MATRIX && u->kind != GB_KIND_MATRIX &&
                take_pending_assign(asg, w, mask, A, u, d, gb_spmv_result_iso(sr, A->iso, u->iso, vxm));
        if (!fused) gb_deferred_resolve(0, nullptr);
    }
    // a pending root that this call cannot consume (below: only the fused notebook level can) is
    // materialised before the views are built: a value mask is resolved into bits of its own
    // there, and one resolved from a pending root's storage would be the empty vector's
    const bool may_take_root = fused && u == w && !accum && d.replace && d.comp && d.structure;
    if (live(GB_DEFER_ROOT) && !may_take_root) root_flush();
    const int64_t hp_t0 = g_hprof_on ? gb_hprof_now() : 0;
    spmv_views V;
    spmv_build_views(V, mask, sr, A, u, d, vxm, a_rows, fused ? &asg : nullptr);
    if (g_hprof_on) gb_hprof_add(2, "do_spmv views+mask", gb_hprof_now() - hp_t0);
    // a pending root (the BFS start): consumed by the notebook level shape -- q<!v.S, replace> =
    // q (+).(x) A with the stamp v<q> = x fused, iso result, push orientation at hand -- whose kernel
    // pushes from it; materialised before any other SpMV
    if (live(GB_DEFER_ROOT)) {
        const bool shape = may_take_root && V.iso_result && V.push && V.push->nrows == u->nrows && V.push->hubs &&
                           gb_knob("spmv_direction") != 1;
        if (shape) asg.root = root_take(u);
        if (asg.root >= 0) {
            // u's storage does not hold the root: its iso value (true) and count come from the host
            V.uv.vals = true_dev();
            V.uv.count = nullptr;
            if (asg.q_iso) asg.q_iso = true_dev();
        } else {
            root_flush();
        }
    }
    gb_vec_result T;
    if (w->kind != GB_KIND_MATRIX) {
        if (!w->pub) w->pub = gb_host_slot_alloc();
        T.pub = w->pub;
        T.pub_seq = gb_next_pub_seq(T.pub);
    }
    {
        GB_HPROF(3, "gb_spmv (host+launch)");
        gb_spmv(T, V.av, V.push, V.uv, V.m, sr, vxm, fused ? &asg : nullptr);
    }
    const void *hint_key = T.hint_key;
    const bool published = T.published;
    GB_HPROF(4, "writeback+epilogue");
    const bool direct = gb_writeback_vector(w, T, mask, d, accum, true);
    if (direct && published) {
        // w's count is the one the kernel published; valid until more work is enqueued
        w->pub_seq = T.pub_seq;
        w->pub_epoch = gb_epoch();
    }
    if (direct && hint_key && w->kind != GB_KIND_MATRIX) {
        w->hint_valid = true;
        w->hint_key = hint_key;
    }
    if (fused) spec_after_level(w, mask, accum, sr, A, u, d, vxm, asg, direct, published);
}

extern "C" {

// the deferred work is adopted, fused or resolved inside (gb_do_spmv)
GrB_Info GrB_mxv(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring op,
                 const GrB_Matrix A, const GrB_Vector u, const GrB_Descriptor desc) {
    return gb_api_impl<GB_DEFER_ALL>(OBJ(w), [&] {
        gb_do_spmv(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(A), gb_obj_check(u),
                   gb_read_desc(desc), false);
    }, __func__);
}

GrB_Info GrB_vxm(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring op,
                 const GrB_Vector u, const GrB_Matrix A, const GrB_Descriptor desc) {
    GB_HPROF(0, "GrB_vxm total");
    return gb_api_impl<GB_DEFER_ALL>(OBJ(w), [&] {
        gb_do_spmv(gb_obj_check(w), gb_obj_check(mask, true), accum, op, gb_obj_check(A), gb_obj_check(u),
                   gb_read_desc(desc), true);
    }, __func__);
}

}  // extern "C"
