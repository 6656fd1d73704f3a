// orbx_resident.h — what the files that work on resident handles share (orbx_resident.hip, orbx_proj.hip, orbx_pose.hip,
// orbx_triangulate.hip, orbx_sim3.hip, orbx_sim3opt.hip, orbx_pnp.hip, orbx_lba.hip, orbx_essential.hip; not part of orbx_internal.h): the frame and map-point handles, the per-thread staging of one call
// (CallCtx: reserve, upload, fetch, the blob cursor), the stream ordering behind a handle's last writer, and the launches of the two
// kernels of orbx_resident.hip that the searches of orbx_proj.hip need.
#pragma once
#include "orbx_internal.h"
#include <shared_mutex>
#include <string.h>
#include <vector>

#define PG_COLS 64 // FRAME_GRID_COLS, include/Frame.h:38
#define PG_ROWS 48 // FRAME_GRID_ROWS, include/Frame.h:37
#define PG_CELLS (PG_COLS * PG_ROWS)

struct DevFrame {
    int n;
    const float *x, *y, *angle, *u_right;
    const int32_t *octave;
    const uint32_t *desc;
    const uint8_t *occupied;
    float min_x, min_y, max_x, max_y, inv_w, inv_h;
};

// ---- the staging of one call: a pinned host blob and its device twin (one upload), a device work area and the pinned block its head is
// downloaded into.  One context per thread and device (the array is orbx_resident.hip's); every capacity is in bytes.
struct CallCtx : ThreadCtx {
    uint8_t *h_blob = nullptr; size_t h_cap = 0;
    uint8_t *d_blob = nullptr; size_t d_cap = 0;
    uint8_t *d_work = nullptr; size_t work_cap = 0;
    uint32_t *d_entries = nullptr; size_t ent_cap = 0;   // the candidate pool of proj_search
    int32_t *h_out = nullptr; size_t out_cap = 0;
    int32_t *h_n = nullptr;    // pinned: the feature count a frame created from extraction outputs reads back
    hipEvent_t ev_a = nullptr, ev_b = nullptr;   // the pair round a launch while a LaunchProfile (below) is on; made on first use
    ORBX_LOCAL void release();
    ~CallCtx() { release(); }
};
ORBX_LOCAL int orbx_call_ctx(int device, CallCtx **out);   // the calling thread's context on `device`, set up (orbx_ctx_enter)

// blob, work area and download block of a call, each grown only when the request exceeds it, then to twice the request (0: not needed)
static inline int call_reserve(CallCtx *c, size_t blob, size_t work, size_t out)
{
    int rc = ORBX_OK;
    if (blob > c->h_cap) rc = ensure_pinned(&c->h_blob, &c->h_cap, 2 * blob);
    if (!rc && blob > c->d_cap) rc = ensure(&c->d_blob, &c->d_cap, 2 * blob);
    if (!rc && work > c->work_cap) rc = ensure(&c->d_work, &c->work_cap, 2 * work);
    if (!rc && out > c->out_cap) rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out);
    return rc;
}
static inline int call_upload(CallCtx *c, size_t blob)
{
    ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    return ORBX_OK;
}
// behind the call's launches: their launch error, the head of the work area into h_out, and the stream drained
static inline int call_fetch(CallCtx *c, size_t out)
{
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, c->d_work, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    return ORBX_OK;
}

// a cursor over a blob: sub-blocks at 16-byte boundaries, `h` where the host writes them and `d` where the device will find them.  Without
// `h` it only counts: put() touches no memory and gives no address.
struct BlobCursor {
    uint8_t *h, *d;
    size_t o;
    size_t take(size_t bytes) { const size_t at = o; o += a16(bytes); return at; }
    uint8_t *put(const void *src, size_t bytes, int absent = 0)   // src == NULL: `bytes` bytes of `absent`
    {
        const size_t at = take(bytes);
        if (!h) return nullptr;
        if (bytes) { if (src) memcpy(h + at, src, bytes); else memset(h + at, absent, bytes); }
        return d + at;
    }
};

// ---- the arrays of the jobs of a batch call (orbx_pose.hip, orbx_sim3opt.hip, orbx_sim3.hip, orbx_pnp.hip).  A solver states a job's arrays
// ONCE, in a function that calls in() for every array that goes up and out() for every array that comes down, in the order they lie in the
// blob and in the download block.  The call walks that function over its jobs three times: to MEASURE (cursors that only count: call_reserve
// gets the sizes the staging will use), to STAGE (the uploads into the blob, the job table's fields set to the device addresses) and, behind
// call_fetch, to DELIVER.  up0 / down0: the bytes in front of the first job's arrays (the job table; the out-records, if any).
struct JobArrays {
    enum Mode { MEASURE, STAGE, DELIVER };
    BlobCursor up, down;   // what a cursor has a base for is what the walk does
    JobArrays(Mode m, CallCtx *c, size_t up0, size_t down0) : up{ nullptr, nullptr, up0 }, down{ nullptr, nullptr, down0 }
    {
        if (m == STAGE) { up.h = c->h_blob; up.d = c->d_blob; down.d = c->d_work; }
        if (m == DELIVER) down.h = (uint8_t *)c->h_out;
    }
    // `field` is written in STAGE alone: only there has `up` a host base (h_blob, never null behind call_reserve), and put() gives an
    // address only from a cursor that has one.  MEASURE and DELIVER count past the array and leave the job they are handed untouched.
    template <class T>
    void in(const T *&field, const void *src, size_t bytes)
    {
        uint8_t *d = up.put(src, bytes);
        if (d) field = (const T *)d;
    }
    // DELIVER: the array goes to dst, where there is one, and the return value is where it was fetched to (else nullptr)
    template <class T>
    const uint8_t *out(T *&field, void *dst, size_t bytes)
    {
        const size_t at = down.take(bytes);
        if (down.d) field = (T *)(down.d + at);
        if (down.h && dst) memcpy(dst, down.h + at, bytes);
        return down.h ? down.h + at : nullptr;
    }
};

// ---- the per-kernel launch profile of a host-driven solver (orbx_debug_lba_profile, orbx_debug_eg_profile; one thread_local object each, N
// its slots): while it is on, every launch of the thread's calls sits between the context's two events and is waited for, and its device
// time goes to its kernel's slot.
template <int N>
struct ORBX_LOCAL LaunchProfile {
    bool on = false;
    double ms[N] = {};
    int32_t n[N] = {};
    // pc, the context to hand to launch(): c with its events made (CallCtx::release gives them back), or nullptr while the profile is off
    int ctx(CallCtx *c, CallCtx **pc) const
    {
        *pc = on ? c : nullptr;
        if (on && !c->ev_a) ORBX_HIP(hipEventCreate(&c->ev_a));
        if (on && !c->ev_b) ORBX_HIP(hipEventCreate(&c->ev_b));
        return ORBX_OK;
    }
    template <class F>
    void launch(int slot, CallCtx *pc, F f)
    {
        if (!pc) { f(); return; }
        float t = 0.f;
        (void)hipEventRecord(pc->ev_a, pc->stream);
        f();
        (void)hipEventRecord(pc->ev_b, pc->stream);
        if (hipEventSynchronize(pc->ev_b) == hipSuccess && hipEventElapsedTime(&t, pc->ev_a, pc->ev_b) == hipSuccess) { ms[slot] += t; n[slot]++; }
    }
    // the entry point: enable != 0 clears and switches on; 0 switches off, hands back what was gathered and returns N
    int entry(int enable, double *ms_out, int32_t *launches)
    {
        if (enable) { *this = LaunchProfile(); on = true; return ORBX_OK; }
        on = false;
        if (ms_out) memcpy(ms_out, ms, sizeof ms);
        if (launches) memcpy(launches, n, sizeof n);
        return N;
    }
};

// workgroups of 256 threads for n items, one at the least
static inline unsigned grid256(int n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// ---- the arrays of a frame, as they lie in a resident frame's block and, up to o_coff, at the head of a host-pointer call's staging
// blob: x[n] y[n] octave[n] angle[n] u_right[n] desc[n][32] | cell_off[3073] cell_idx[n]
struct FrameLayout { size_t o_x, o_y, o_oct, o_ang, o_ur, o_desc, o_coff, o_cidx, bytes; };

static inline FrameLayout frame_layout(size_t nc)
{
    FrameLayout L;
    BlobCursor b = { nullptr, nullptr, 0 };
    L.o_x = b.take(4 * nc); L.o_y = b.take(4 * nc); L.o_oct = b.take(4 * nc); L.o_ang = b.take(4 * nc); L.o_ur = b.take(4 * nc);
    L.o_desc = b.take(32 * nc); L.o_coff = b.take(4 * (PG_CELLS + 1)); L.o_cidx = b.take(4 * nc);
    L.bytes = b.o;
    return L;
}

// the DevFrame of n features laid out by L behind `base` (a device address), image bounds b = min_x, min_y, max_x, max_y; occupied is
// the search's to set
static inline DevFrame dev_frame(const uint8_t *base, const FrameLayout &L, int n, const float b[4])
{
    DevFrame F;
    F.n = n; F.x = (const float *)(base + L.o_x); F.y = (const float *)(base + L.o_y); F.octave = (const int32_t *)(base + L.o_oct);
    F.angle = (const float *)(base + L.o_ang); F.u_right = (const float *)(base + L.o_ur); F.desc = (const uint32_t *)(base + L.o_desc);
    F.occupied = nullptr;
    F.min_x = b[0]; F.min_y = b[1]; F.max_x = b[2]; F.max_y = b[3];
    F.inv_w = (float)PG_COLS / (b[2] - b[0]);  // src/Frame.cc:164-165
    F.inv_h = (float)PG_ROWS / (b[3] - b[1]);
    return F;
}

// a host-pointer frame's arrays into the head of the staging blob (frame_layout(n).o_coff bytes); the DevFrame addresses them where the
// upload of the blob will put them
static inline DevFrame frame_stage(CallCtx *c, const orbx_frame_feats *cur)
{
    const size_t nc = (size_t)cur->n;
    const FrameLayout L = frame_layout(nc);
    uint8_t *h = c->h_blob;
    memcpy(h + L.o_x, cur->x, 4 * nc); memcpy(h + L.o_y, cur->y, 4 * nc); memcpy(h + L.o_oct, cur->octave, 4 * nc);
    if (cur->angle) memcpy(h + L.o_ang, cur->angle, 4 * nc); else memset(h + L.o_ang, 0, 4 * nc);
    memcpy(h + L.o_ur, cur->u_right, 4 * nc); memcpy(h + L.o_desc, cur->desc, 32 * nc);
    const float b[4] = { cur->min_x, cur->min_y, cur->max_x, cur->max_y };
    return dev_frame(c->d_blob, L, cur->n, b);
}

// ---- the resident frame (include/orbx.h: orbx_frame).  Its block comes from the frame pool of orbx_resident.hip.
struct FrameBlock { uint8_t *d = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; };

struct orbx_frame : FrameLayout {   // the block's layout: frame_layout(n)
    int device, n, has_angle;
    float bounds[4];   // min_x, min_y, max_x, max_y
    FrameBlock blk;
    bool pending;   // the creation may still be running: a call waits for blk.ev on its own stream (frame_order_before); only the
                    // per-frame searches, which own the frame, clear it once they have synchronised
    std::vector<int32_t> h_oct;   // a frame made from host pointers keeps its octaves: orbx_frame_pose_optimize checks them before any device work
    // orbx_frame_set_depth: mvDepth and the raw positions in one allocation of the frame's own (raw == nullptr: x / y); has_stereo = some
    // u_right >= 0 as far as the host saw them, from_extraction = it saw none
    float *d_depth = nullptr, *d_raw_x = nullptr, *d_raw_y = nullptr;
    bool depth_set = false, has_stereo = false, from_extraction = false;
};

static inline DevFrame frame_dev(const orbx_frame *f) { return dev_frame(f->blk.d, *f, f->n, f->bounds); }

// stream s behind the frame's creation, ordered by its event (no device synchronisation); the handle is not written
static inline int frame_order_before(const orbx_frame *f, hipStream_t s)
{
    if (f->pending) ORBX_HIP(hipStreamWaitEvent(s, f->blk.ev, 0));
    return ORBX_OK;
}

// ---- the resident map-point table (include/orbx.h: orbx_mappoints).  ONE device allocation made at creation: geom[capacity][8] |
// desc[capacity][32] | the staging of one upload of orbx_mappoints_set, MP_STAGE_RECORDS records at most (a larger set goes in several
// uploads); nothing grows.  An upload is packed by its own record count, slots[k] | geom[k][8] | desc[k][32] with a half not given left
// out, so what crosses PCIe is 4 + 32 or 4 + 64 bytes per record sent, whatever the capacity.
// Host state: which halves every slot has been given, and the event of the most recent _set.  A _set holds `mu` exclusively while it
// enqueues, a search holds it shared until its stream has drained: a slot is never rewritten under a search in flight, and a search on
// another stream than the _set's waits for the event, not for the device.
struct orbx_mappoints {
    int device, capacity;
    uint8_t *d_blob;
    float4 *d_geom; uint4 *d_desc;
    uint8_t *d_stage, *h_stage;          // h_stage: pinned, as large as d_stage
    int stage_records; size_t st_bytes;  // records one upload holds; bytes of the staging
    std::vector<uint8_t> have;           // bit 0: geom given, bit 1: desc given; 3 = set
    std::vector<uint32_t> stamp; uint32_t gen;   // duplicate slots of one _set
    mutable hipEvent_t ev; mutable hipStream_t ev_stream; mutable bool ev_set;
    mutable std::shared_timed_mutex mu;
};

// stream s behind the table's most recent _set (the caller holds m->mu shared)
static inline int mappoints_order_before(const orbx_mappoints *m, hipStream_t s)
{
    if (m->ev_set && m->ev_stream != s) ORBX_HIP(hipStreamWaitEvent(s, m->ev, 0));
    return ORBX_OK;
}

// ---- what orbx_proj.hip needs of orbx_resident.hip's kernels
// Frame::AssignFeaturesToGrid of a host-pointer frame (k_grid_build): cell_off[PG_CELLS + 1], cell_idx[F.n]
ORBX_LOCAL void orbx_grid_build_launch(const DevFrame &F, int *d_cell_off, int *d_cell_idx, hipStream_t s);
// Frame::isInFrustum from a pose (k_frustum).  thr[k] is the smallest float r with ceilf(logf(r) / mfLogScaleFactor) > k.
struct FrustumArgs {
    float R[9], t[3], Ow[3];
    float fx, fy, cx, cy, mbf, min_x, min_y, max_x, max_y;
    float view_cos_limit;
    int nlevels;
    float thr[ORBX_MAX_LEVELS - 1];   // [nlevels - 1] used
};
// what k_frustum writes: the arrays of a dense DevPoints (aux = xr, valid = in_view).  has_obs / desc are NULL for orbx_mappoints_frustum.
struct FrustumOut {
    float *u, *v, *xr, *view_cos;
    int32_t *level;
    uint8_t *in_view, *has_obs;
    uint4 *desc;
};
// the refusals of a frustum call, before any launch, and its kernel arguments.  any_bit: which bit pattern of flags[i] makes point i
// eligible (orbx_mappoints_frustum: any non-zero byte; the fused search: bit 0)
ORBX_LOCAL int orbx_frustum_args(const char *who, const orbx_mappoints *m, const int32_t *slots, const uint8_t *flags, int n, bool any_bit,
                                 const float *pose, const float *cam, float view_cos_limit, float lsf, int nlevels, FrustumArgs *A);
// k_frustum over n points of table m; d_slots / d_flags are device addresses
ORBX_LOCAL void orbx_frustum_launch(const orbx_mappoints *m, const int32_t *d_slots, const uint8_t *d_flags, int n, const FrustumArgs &A,
                                    const FrustumOut &o, hipStream_t s);
