// orbx_internal.h — shared host/device definitions of liborbx (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/orbx.h"

#define ORBX_MAX_LEVELS 16
#define ORBX_MAX_DEVICES 16   // the per-thread context arrays have this size: the per-call searches refuse a device index at or beyond it
#define ORBX_EDGE 19          // EDGE_THRESHOLD, reference src/ORBextractor.cc:74
#define ORBX_MIN_BORDER 16    // EDGE_THRESHOLD-3, src/ORBextractor.cc:934
#define ORBX_TILE_PITCH 80    // LDS pitch of a FAST cell tile when a cell is wider than 38 px (cell side <= 59 + 6 halo + 1): 3 rows per direct load
#define ORBX_SCORE_PITCH 64   // LDS pitch of a FAST cell score tile (detect side <= 59 + 2)
#define ORBX_MAX_DIM 4096     // packed candidate = x | y<<12 | score<<24
#define ORBX_NODE_BITS 14     // quadtree node id bits inside the per-point label
#define ORBX_CAND_PRIM 16      // a cell's first candidates live in a dense 64-byte record (cells contiguous); only the overflow uses its big slot block
#ifndef ORBX_TREE_REG_PTS
#define ORBX_TREE_REG_PTS 3072 // k_tree: a level with at most this many candidates keeps them in registers (12 per thread of 256)
#endif
#define ORBX_TREE_REG_PTS_BIG 4096 // the same for the 1024-thread form (4 per thread)
#ifndef ORBX_TREE_OVER_PTS
#define ORBX_TREE_OVER_PTS 1024 // register form: points of a level beyond the register capacity that an LDS overflow array takes
#endif
#define ORBX_LAUNCH_FORM_FIELDS 10 // orbx_debug_launch_forms: pyramid regime, FAST waves + grid order, quadtree threads / tables / register mode, k_desc levels, stereo kpw / XCD grid, k_desc row pass
#define ORBX_FAST_LIST_CAP 512 // k_fast: pretest candidates listed per round (u16 each); denser cells take several rounds

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline size_t a16(size_t v) { return align_up(v, 16); }   // the sub-block alignment of every staging blob

// Geometry of one pyramid level for one image size (host computes, device reads).
struct LevelGeom {
    int w, h, pitch;        // pitch in bytes of the stored level (levels >= 1)
    long long pyr_off;      // byte offset of the level inside one image's pyramid block (levels >= 1)
    int n_cols, n_rows, w_cell, h_cell; // FAST cell grid, src/ORBextractor.cc:944-951
    int cell_base, n_cells; // index range of this level's cells in the per-image cell arrays
    int cand_cap;           // candidate slots per cell
    long long cand_off;     // first slot (u32 units) of this level in the per-image candidate block
    int quota;              // mnFeaturesPerLevel
    int n_ini; float hx;    // quadtree roots, src/ORBextractor.cc:627-628
    int tree_w, tree_h;     // maxBorder - minBorder
    int node_cap;           // max simultaneous quadtree leaves (+slack)
    int kp_off, kp_cap;     // slot range in the per-image per-level keypoint staging
    float scale;            // mvScaleFactor[level]
    int patch_size;         // (int)(31*scale)
    int tab_x, tab_y;       // offsets (int16 units) of the resize tables [ofs|c0|c1] x 3*w / 3*h
    int tab_tx, tab_ty;     // offsets of k_resize's per-tile-column / per-tile-row records
    int resize_lds;         // 1: k_resize's LDS tile fits this level's scale, 0: k_resize_direct, 2: exact 2x -> area average (k_resize_direct)
};

struct Geom {
    int nlevels, w, h;
    int total_cells;        // per image
    long long cand_total;   // per image, u32 units
    int kp_total;           // per image staging slots
    long long pyr_bytes;    // per image, levels >= 1
    int max_cells_level;    // max n_cells over levels
    int max_node_cap;
    int fast_lds_sc, fast_lds_list, fast_lds_bm, fast_bm_rows, fast_lds_bytes; // LDS carve of k_fast
    int fast_small;         // 1: k_fast<48,40> (every cell <= 38 px wide), 0: k_fast<80,64>
    int fast_list_cap_big, fast_lds_bm_big, fast_lds_bytes_big;   // the carve with a candidate list that holds a whole cell (several waves per cell)
    int fast_lane_tab_off;  // k_fast's lane table (one block of 64 x 16 bytes per detect shape): byte offset behind the first cell record
    int fast2_ok, total_pairs;   // k_fast2 (a wave per pair of adjacent cells) is usable for this geometry; pair records per image
    int fast2_first[2], fast2_count[2];   // two launches: levels whose detect areas have at most 32 rows, then the taller ones
    int fast2_lds_sc[2], fast2_lds_list[2], fast2_lds_bm[2], fast2_bm_rows[2], fast2_lds_bytes[2];
    LevelGeom lv[ORBX_MAX_LEVELS];
};

// Per-cell record of k_fast (same for every image): one 32-byte scalar load replaces the level search
// and the cell-grid arithmetic (a chain of dependent scalar loads per wave).
struct CellRec {
    short level, skip;
    short ini_x, ini_y, tw, th;  // cell rectangle incl. 3-px halo, level coordinates
    int pitch;                   // level pitch (levels >= 1; level 0 uses the caller's pitch)
    int cand_cap;
    unsigned gpr_magic;          // 0xFFFFFFFF / gpr + 1, gpr = dword groups per detect row = (tw - 6 + 3) >> 2: multiply-high division by gpr
    long long pyr_off;           // byte offset of the level in one image's pyramid block
    long long cand_slot;         // first candidate slot (u32 units) of this cell in one image's block
};
static_assert(sizeof(CellRec) == 40, "CellRec layout");

struct ProfEvent { hipEvent_t a, b; int stage; bool owns_a; };

// One frame in flight of the pipelined host-pointer stereo path (orbx_extract_stereo_submit / _wait)
struct PipeSlot {
    uint8_t *h_in, *d_in; size_t h_in_cap, d_in_cap;   // both eyes, pinned host staging and device level 0
    uint8_t *h_in_dev, *h_out_dev;           // the addresses a kernel reads / writes the two pinned buffers at
    uint8_t *h_out; size_t h_out_cap;        // pinned result block: orbx_result_layout(2, need)
    uint8_t *d_out; size_t d_out_cap;        // one device block in the layout of h_out (a single download per frame)
    void *d_kps, *d_desc, *d_n; float *d_ur, *d_z;   // views into d_out
    hipEvent_t ev_h2d, ev_done, ev_d2h;      // input landed / kernels finished / results landed in h_out
    int cap, ticket, eyes; bool busy;       // eyes: 1 mono, 2 stereo, ORBX_PIPE_RGBD (one image + its depth)
    struct orbx_extractor *lane;             // the kernel lane (the handle or its shadow) that ran the slot's frame
};

// Byte layout of the block a host-pointer call's results land in (the pinned h_out of the synchronous forms; a pipeline slot's d_out and
// h_out, always with images == 2): [counts | keypoints x images | descriptors x images | uRight | depth | xy], `need` entries per image.
struct ResultLayout { size_t kps, desc, ur, z, xy, bytes; };   // the counts are ints at offset 0; a pipelined frame's kernel error flag is int index 2
static inline ResultLayout orbx_result_layout(int images, int need)
{
    const size_t n = (size_t)need, col = align_up(4 * n, 64);
    ResultLayout L;
    L.kps = align_up(sizeof(int) * ((size_t)images + 1), 64);
    L.desc = L.kps + align_up(sizeof(orbx_keypoint) * n * images, 64);
    L.ur = L.desc + align_up(32 * n * images, 64);
    L.z = L.ur + col;
    // a pipeline slot always holds two images: an RGB-D frame, which extracts one, keeps its xy rows in the unused second-eye keypoint rows
    L.xy = images == 2 ? L.kps + align_up(sizeof(orbx_keypoint) * n, 64) : L.z + col;
    L.bytes = images == 2 ? L.z + col : L.xy + 8 * n;
    return L;
}
#define ORBX_PIPE_DEPTH 4
#define ORBX_PIPE_RGBD 3                     // PipeSlot::eyes of an RGB-D frame

struct orbx_extractor {
    int device;
    int nfeatures, nlevels, ini_th, min_th;
    double scale_factor;
    int max_w, max_h, max_batch;
    float sf[ORBX_MAX_LEVELS], isf[ORBX_MAX_LEVELS], sig2[ORBX_MAX_LEVELS], isig2[ORBX_MAX_LEVELS];
    int quota[ORBX_MAX_LEVELS];
    int umax[16];
    int cv_profile, gauss[4];        // OpenCV generation whose GaussianBlur taps k_desc filters with (orbx_extractor_set_cv_profile)

    hipStream_t stream;
    hipStream_t last_launch_stream;  // stream of the most recent kernel launches on this handle's workspaces (caller's or `stream`)
    hipEvent_t ev_switch;            // orders a launch on a new stream behind the work of the previous one (orbx_use_stream)
    // geometry of the current image size
    Geom geom;           // host copy (geom.w == 0: none yet)
    Geom *d_geom;        // device copy
    int16_t *d_tabs; size_t tabs_cap;      // resize tables
    CellRec *d_cells; size_t cells_cap;    // per-cell records of k_fast
    void *d_pairs; size_t pairs_cap;       // per-pair records of k_fast2 (PairRec, orbx_fast.hip)
    int last_fast_form;                    // debug: 1 = k_fast, 2 = k_fast2 ran in the most recent extraction
    int32_t last_forms[ORBX_LAUNCH_FORM_FIELDS]; // debug: launch forms of the most recent extraction / stereo launch (orbx_debug_launch_forms)
    int fast_pair;                         // ORBX_FAST_PAIR: 1 = k_fast2 wherever the geometry allows it, 0 (default) = never
    int desc_valu_rowpass;                 // ORBX_DESC_VALU_ROWPASS: 1 = k_desc's row pass on the vector ALUs, 0 (default) = on the matrix cores
    // workspace (sized for max_w x max_h x max_batch)
    uint8_t *d_pyr; size_t pyr_cap;        // levels >= 1, all images
    uint8_t *d_stage_in; size_t stage_in_cap; // host-API input staging (level 0)
    int *d_cell_cnt; size_t cell_cnt_cap;
    uint32_t *d_cand; size_t cand_cap;
    uint32_t *d_cand_prim; size_t cand_prim_cap;   // [max_batch][total_cells][ORBX_CAND_PRIM]
    uint32_t *d_tree_pts; size_t tree_pts_cap; uint16_t *d_tree_nid; size_t tree_nid_cap; // overflow scratch of the quadtree
    unsigned char *d_tree_tab; size_t tree_tab_cap; // quadtree node tables of configurations whose tables exceed the LDS (else unused)
    int *d_lvl_cnt;                        // [max_batch][nlevels]
    uint32_t *d_lvl_kp; size_t lvl_kp_cap; // [max_batch][kp_total]
    // host-API pinned staging (pageable 2-D copies cost milliseconds)
    uint8_t *h_stage_in; size_t h_stage_in_cap;
    uint8_t *h_out; size_t h_out_cap;
    int *h_flag;                           // pinned copy of the kernel error flag
    // host-API output staging
    void *d_out_kps, *d_out_desc, *d_out_n; int out_cap; int out_batch;
    float *d_out_ur, *d_out_depth;
    // stereo scratch
    int *d_st_dist; size_t st_cap;         // SAD per left keypoint (or -1)
    void *d_st_entries; size_t st_ent_cap;  // row table entries of k_stereo_prep (one uint4 per right keypoint, see orbx_stereo.hip)
    void *scratch[10]; size_t scratch_cap[10]; // host-API upload buffers (8, 9: orbx_extract_rgbd's depth image and undistorted positions)
    // pipelined stereo frames: copies ride their own streams so that frame i+1 uploads and frame i-1 downloads while frame i computes
    PipeSlot pipe[ORBX_PIPE_DEPTH]; hipStream_t copy_in, copy_out; unsigned pipe_next;
    int pipe_warm_w, pipe_warm_h;    // the image size every lane / slot of the pipelined forms has been run on once (orbx_pipeline_warm); 0 = none yet
    int pipe_rgbd_warm_w, pipe_rgbd_warm_h;   // ... and through the RGB-D mode (its larger input block, k_gray, k_rgbd_depth); 0 = none yet
    bool pipe_rgbd_gather;           // RGB-D depth transport: k_rgbd_depth reads the pinned host depth in place (default) or the slot's upload (ORBX_PIPE_RGBD_GATHER=0)
    bool pipe_counted;               // this handle is counted in the process-wide number of pipelined handles
    orbx_extractor *lanes[ORBX_PIPE_DEPTH - 1];   // further kernel lanes of the pipelined forms (shadow handles with their own stream and
                                     // workspaces): submission i runs on lane i % pipe_lanes, so the launch chains of neighbouring frames
                                     // overlap (a frame alone fills a few percent of the chip)
    int pipe_lanes;                  // lanes in use (1 .. ORBX_PIPE_DEPTH; ORBX_PIPE_LANES)
    bool pipe_inline;                // a frame's upload and download ride its lane's stream (no copy streams, no events between them)
    bool pipe_kcopy;                 // ... and are done by a copy kernel reading / writing the pinned buffers over PCIe (inline form only)
    int *flag_out;                   // where the next extraction's k_desc drops the kernel error flag (pipelined frames: into the slot's block)
    // grouped pyramid of small launches (k_pyr_group): group i builds levels first .. first + n - 1 in one launch
    struct PyrGroup { int first, n, tiles_x, tiles_y, tab_cx, tab_cy, lds_b, lds_bytes; } pyr_groups[ORBX_MAX_LEVELS];
    int n_pyr_groups;                // 0: this geometry has no grouped form (per-level launches at every batch size)
    int pyr_group_max_images;        // launches of at most this many images take the grouped form
    int pyr_group_mid_images;        // ... and up to this many: levels of the first group by one launch each, the later groups grouped
    int pyr_group_mid_cfg;           // the configured value of pyr_group_mid_images (default 24 / ORBX_PYR_GROUP_MID_IMAGES): what a non-zero group limit restores
    int stereo_kpw_forced;           // ORBX_STEREO_KPW (1 / 4), read once when the handle is created: forces k_stereo's keypoints per wave; 0 = by launch size
    int fast_waves;                  // waves per FAST cell: 0 = by launch size (several for a frame or two, one for batches); 1-4 forces (ORBX_FAST_WAVES)
    // stereo row table written by the most recent extraction as a by-product of k_desc (desc_rowtab): valid for the keypoint buffer
    // rt_kps (capacity rt_cap per image, rt_batch images); d_rt_off == nullptr: this geometry has none (more rows than k_desc's LDS holds)
    int *d_rt_off; size_t rt_off_cap; uint8_t *d_rt_entries; size_t rt_entries_cap; int rt_ent_cap;
    const void *rt_kps; int rt_cap, rt_batch;
    int *d_st_arrive;                // per stereo pair: workgroups of k_stereo that have finished (the last one applies the median cut)
    // state of the most recent extract
    const uint8_t *last_img0; size_t last_img_stride, last_pitch; int last_batch;
    // profiling
    bool prof, prof_chain; unsigned prof_mask; hipStream_t prof_last_stream; std::vector<ProfEvent> prof_ev; std::vector<hipEvent_t> prof_pool;
    float prof_ms[ORBX_STAGE_COUNT]; int prof_n[ORBX_STAGE_COUNT];
};

// one side of a BoW search on the device (FeatureVector as CSR, see orbx_featset)
struct DevFeat {
    int n, nnodes;
    const uint32_t *desc;     // [n][8]
    const uint32_t *node_id;  // [nnodes]
    const int32_t *node_off;  // [nnodes+1]
    const uint32_t *feat;
    const uint8_t *flag;
    const float *angle, *x, *y, *u_right;
    const int32_t *octave;
    const uint32_t *sdesc;    // [len(feat)][8] descriptors in list order (desc[feat[k]])
    const uint8_t *sflag;     // [len(feat)] flags in list order
};

// device-resident BoW data of a batch of frames (orbx_bow_transform_batch_device -> orbx_bowdb_search_batch_device)
struct orbx_bow_frames {
    int device, batch, cap, npad;
    uint8_t *d_buf;
    uint32_t *word_id; double *word_w; uint32_t *node_id;      // [batch][cap]
    uint32_t *bow_id; double *bow_val; int *counts;             // [batch][cap], [batch][cap], [batch][2] (nbow, nnodes)
    uint32_t *fv_node_id; int32_t *fv_node_off; uint32_t *fv_feat; // [batch][cap], [batch][cap+1 -> stride cap+4], [batch][npad]
    float *angle;                                               // [batch][cap]
    uint32_t *sdesc; uint8_t *sflag;                            // [batch][npad][8], [batch][npad]: list-order copies
    DevFeat *d_feats;                                           // [batch]
    uint8_t *h_buf; size_t h_cap;                               // pinned staging of orbx_bow_frames_read
    hipStream_t last_stream;                                    // stream of the most recent transform: the default of read / search
};

void orbx_set_error(const char *fmt, ...);
// orbx_bow.hip: CSR / pointer validation of a feature set; the legacy SearchByBoW kernels behind orbx_match.hip's entry points;
// the form forced by orbx_debug_set_bow_form (0 = none)
int orbx_feat_validate(const orbx_featset *f, int need_geom, int need_flag);
int orbx_bow_run_legacy(int mode, int device, const orbx_featset *as, int na, const orbx_featset *b,
                        float nnratio, int check_ori, int32_t *match, int *nmatches);
int orbx_bow_forced_form();
#define ORBX_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    orbx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return ORBX_E_HIP; } } while (0)

// grow a device / a pinned host buffer to at least `need` bytes (never shrinks it; the old contents are dropped).  On every return path,
// failure included, *cap is at most what *p holds and *p == nullptr implies *cap == 0: a failed growth can never leave a stale
// capacity next to a null pointer for the next, smaller request to write through.
template <class T>
static inline int ensure(T **p, size_t *cap, size_t need)
{
    if (need <= *cap && *p) return ORBX_OK;
    if (*p) ORBX_HIP(hipFree(*p));
    *p = nullptr; *cap = 0;
    if (hipError_t e = hipMalloc((void **)p, need ? need : 16)) { *p = nullptr; orbx_set_error("hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); return ORBX_E_HIP; }
    *cap = need;
    return ORBX_OK;
}
template <class T>
static inline int ensure_pinned(T **p, size_t *cap, size_t need, unsigned flags = hipHostMallocDefault)
{
    if (need <= *cap && *p) return ORBX_OK;
    if (*p) ORBX_HIP(hipHostFree(*p));
    *p = nullptr; *cap = 0;
    if (hipError_t e = hipHostMalloc((void **)p, need ? need : 16, flags)) { *p = nullptr; orbx_set_error("hipHostMalloc(%zu) failed: %s", need, hipGetErrorString(e)); return ORBX_E_HIP; }
    *cap = need;
    return ORBX_OK;
}

// hipSetDevice only when the calling thread is on another device (a read of the thread's current device is cheaper than the set, and the
// hot host paths -- a pipelined submit makes three API entries per frame -- call it every time)
static inline hipError_t orbx_use_device(int device)
{
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return hipSuccess;
    return hipSetDevice(device);
}

// ORBX_OK, or ORBX_E_NO_DEVICE with the one message every entry point gives for a device index that names no visible device
int orbx_check_device(int device);

// What a thread needs to run per-call searches on one device: its own stream.  The four families (MatchCtx orbx_match.hip, BowCtx
// orbx_bow.hip, CallCtx orbx_resident.h / orbx_resident.hip, FrameCtx orbx_frame.hip) derive from it, add their staging buffers, and keep one thread_local array
// [ORBX_MAX_DEVICES] each.  Each has release(): orbx_ctx_leave, then -- if that says so -- its buffers freed, then every pointer and
// capacity reset; and a destructor calling release(), so a thread that ends gives everything back.
struct ThreadCtx { int device = -1; hipStream_t stream = nullptr; };
// c = the thread's slot for `device` (nullptr: device outside [0, ORBX_MAX_DEVICES)).  A set-up context only makes `device` current (no
// device-count query in the steady state); otherwise the device is checked, made current and the non-blocking stream created.
int orbx_ctx_enter(ThreadCtx *c, int device);
// Synchronises and destroys the stream of a set-up context.  Returns whether the caller may free its buffers: false when the context was
// never set up, or when the runtime is already shutting down (HIP is then left alone).
bool orbx_ctx_leave(ThreadCtx *c);
template <class C>
static inline int orbx_ctx_get(C (&slots)[ORBX_MAX_DEVICES], int device, C **out)
{
    C *c = device >= 0 && device < ORBX_MAX_DEVICES ? &slots[device] : nullptr;
    const int rc = orbx_ctx_enter(c, device);
    if (rc == ORBX_OK) *out = c;
    return rc;
}
void orbx_match_thread_release();   // the calling thread's contexts of one family, every device (orbx_thread_release walks the four)
void orbx_bow_thread_release();
void orbx_proj_thread_release();    // (the CallCtx family)
void orbx_frame_thread_release();

// host-side exact arithmetic helpers shared by the .hip files
static inline int orbx_cv_round(float v) { return (int)lrintf(v); }

int orbx_prepare_geometry(orbx_extractor *e, int w, int h);
// The extractor's four stages, one file each (file map: orbx_extract.hip).  A plan is the stage's step of orbx_prepare_geometry: it turns the
// level geometry into the stage's host tables and LDS sizes, and the plans run in this order (k_pyr_group's tables read the finished resize
// tables, k_fast2's pair records the finished cells).  A launch enqueues the stage for the handle's current geometry on stream s and notes
// the form it chose in e->last_forms.  New internal functions stay out of the library's dynamic symbol table.
#define ORBX_LOCAL __attribute__((visibility("hidden")))
struct PyrRef;
ORBX_LOCAL void orbx_pyramid_plan(orbx_extractor *e, Geom &G, std::vector<int16_t> &tabs);
ORBX_LOCAL void orbx_pyramid_launch(orbx_extractor *e, const PyrRef &pr, int batch, hipStream_t s);
ORBX_LOCAL void orbx_fast_plan(const orbx_extractor *e, Geom &G, std::vector<CellRec> &cells, std::vector<uint8_t> &pair_bytes);
ORBX_LOCAL void orbx_fast_launch(orbx_extractor *e, const PyrRef &pr, int batch, hipStream_t s);
ORBX_LOCAL int orbx_tree_plan(const Geom &G, size_t *hbm_tab_bytes);
ORBX_LOCAL int orbx_tree_commit(const Geom &G);
ORBX_LOCAL void orbx_tree_launch(orbx_extractor *e, int batch, hipStream_t s);
ORBX_LOCAL int orbx_desc_upload_constants(orbx_extractor *e);
ORBX_LOCAL bool orbx_desc_rowtab_plan(const Geom &G);
ORBX_LOCAL void orbx_desc_launch(orbx_extractor *e, const PyrRef &pr, int batch, void *d_kps, void *d_desc, void *d_n_out, int cap, hipStream_t s);
#ifdef ORBX_DIAG    // each file's half of orbx_diag_spans
ORBX_LOCAL int orbx_fast_diag_spans(unsigned *out, int reset);
ORBX_LOCAL int orbx_desc_diag_spans(unsigned *out, int reset);
#endif
// the kernel error flag: the int behind the level counts (set by k_tree, handed on by k_desc, read and cleared by orbx_sync)
static inline int *orbx_err_flag(const orbx_extractor *e) { return e->d_lvl_cnt + (size_t)e->max_batch * ORBX_MAX_LEVELS; }
void orbx_prof_begin(orbx_extractor *e, int stage, hipStream_t s);
void orbx_prof_end(orbx_extractor *e, hipStream_t s);
int orbx_ensure_out_staging(orbx_extractor *e, int batch, int cap);
int orbx_scratch(orbx_extractor *e, int slot, size_t bytes, void **out);
// waits for everything launched on this handle's workspaces (its own stream and the caller stream of the most recent
// launches): called before any geometry rebuild or workspace reallocation, so tables are never rewritten and buffers
// never freed under running kernels
int orbx_quiesce(orbx_extractor *e);
void orbx_pipe_handle_released();
// the handle's workspaces are about to be used by launches on stream s: if the previous launches went to another stream, s first
// waits for them (an event, no host synchronisation); records s as the handle's stream
int orbx_use_stream(orbx_extractor *e, hipStream_t s);

// level-0 / level-l pixel pointer of image b (device side helper)
struct PyrRef {
    const uint8_t *img0; long long img0_stride; int img0_pitch;
    const uint8_t *pyr; long long pyr_stride;
};
__device__ __forceinline__ const uint8_t *orbx_level_ptr(const PyrRef &p, const LevelGeom &L, int level, int b, int *pitch)
{
    if (level == 0) { *pitch = p.img0_pitch; return p.img0 + (long long)b * p.img0_stride; }
    *pitch = L.pitch;
    return p.pyr + (long long)b * p.pyr_stride + L.pyr_off;
}
