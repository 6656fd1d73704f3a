// orbx_extract.hip — ORB extractor for gfx950 (MI355X): the handle, the geometry of an image size and the launch sequence.
//
// Replaces ORBextractor::operator() (reference src/ORBextractor.cc:1261-1339) and everything it
// calls; bit-exact contract in SURVEY.md Appendix A/B.  Written for wave64 / LDS staging; all
// arithmetic is integer except fastAtan2 / the pattern rotation (fp32, contraction off) and the
// shared fp64 sincos.  One launch covers a whole batch of images (grid.y = image).
//
// File map: a stage's kernels, the host plan that builds their tables and LDS sizes from Geom, and their launch live in one file each, so
// that a change to one stage cannot move another stage's code (k_fast is sensitive to where its code lies):
//   orbx_pyramid.hip  k_resize, k_resize_direct, k_pyr_group   orbx_pyramid_plan, orbx_pyramid_launch
//   orbx_fast.hip     k_fast, k_fast2                          orbx_fast_plan, orbx_fast_launch
//   orbx_tree.hip     k_tree                                   orbx_tree_plan, orbx_tree_commit, orbx_tree_launch
//   orbx_desc.hip     k_desc (+ the stereo row table)          orbx_desc_upload_constants, orbx_desc_rowtab_plan, orbx_desc_launch
// This file calls the plans from orbx_prepare_geometry in the order of their dependencies and the launches from orbx_extract_batch_device;
// it names no kernel, argument struct or LDS size of theirs.
#include "orbx_device.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int orbx_prepare_geometry(orbx_extractor *e, int w, int h)
{
    if (e->geom.w == w && e->geom.h == h) return ORBX_OK;
    if (w > e->max_w || h > e->max_h || w > ORBX_MAX_DIM || h > ORBX_MAX_DIM) {
        orbx_set_error("image %dx%d exceeds the extractor's maximum %dx%d", w, h, e->max_w, e->max_h);
        return ORBX_E_INVALID;
    }
    Geom G;
    memset(&G, 0, sizeof G);
    G.nlevels = e->nlevels; G.w = w; G.h = h;
    for (int l = 0; l < e->nlevels; l++) {
        LevelGeom &L = G.lv[l];
        L.w = orbx_cv_round((float)w * e->isf[l]);   // src/ORBextractor.cc:1353
        L.h = orbx_cv_round((float)h * e->isf[l]);
        const int min_b = ORBX_MIN_BORDER, max_bx = L.w - ORBX_EDGE + 3, max_by = L.h - ORBX_EDGE + 3;
        const float width = (float)(max_bx - min_b), height = (float)(max_by - min_b);
        if (max_bx - min_b < 30 || max_by - min_b < 30) {
            orbx_set_error("level %d (%dx%d) is smaller than one 30-px FAST cell", l, L.w, L.h);
            return ORBX_E_TOO_SMALL;
        }
        L.n_cols = (int)(width / 30.f);               // :946-951
        L.n_rows = (int)(height / 30.f);
        L.w_cell = (int)ceilf(width / L.n_cols);
        L.h_cell = (int)ceilf(height / L.n_rows);
        if (L.w_cell > 59 || L.h_cell > 59) { orbx_set_error("internal: cell larger than 59"); return ORBX_E_INVALID; }
        L.n_cells = L.n_cols * L.n_rows;
        L.cell_base = G.total_cells;
        G.total_cells += L.n_cells;
        L.cand_cap = ((L.w_cell + 1) / 2) * ((L.h_cell + 1) / 2); // strict 3x3 maxima cannot be adjacent
        L.cand_off = G.cand_total;
        G.cand_total += (long long)L.n_cells * L.cand_cap;
        L.quota = e->quota[l];
        L.tree_w = max_bx - min_b; L.tree_h = max_by - min_b;
        L.n_ini = (int)roundf((float)L.tree_w / L.tree_h); // :627
        if (L.n_ini < 1) { orbx_set_error("level %d: aspect ratio gives zero quadtree roots (reference divides by zero)", l); return ORBX_E_TOO_SMALL; }
        L.hx = (float)L.tree_w / L.n_ini;                  // :628
        int nc = L.quota + 3 > 4 * L.n_ini ? L.quota + 3 : 4 * L.n_ini;
        L.node_cap = (nc + 4 + 3) & ~3;
        if (L.node_cap >= (1 << ORBX_NODE_BITS)) {
            orbx_set_error("level %d asks for %d features: the quadtree labels hold %d leaves per level (nfeatures <= ~%d at scale factor 1.2)",
                           l, L.quota, (1 << ORBX_NODE_BITS) - 8, 70000);
            return ORBX_E_INVALID;
        }
        L.kp_cap = L.node_cap; L.kp_off = G.kp_total; G.kp_total += L.kp_cap;
        L.scale = e->sf[l];
        L.patch_size = (int)(31 * e->sf[l]);               // :1023
        if (l >= 1) {
            L.pitch = (int)align_up(L.w, 64);
            L.pyr_off = G.pyr_bytes;
            G.pyr_bytes += (long long)L.pitch * L.h;
        }
        if (L.n_cells > G.max_cells_level) G.max_cells_level = L.n_cells;
        if (L.node_cap > G.max_node_cap) G.max_node_cap = L.node_cap;
    }
    G.pyr_bytes = (long long)align_up((size_t)G.pyr_bytes, 256);
    // the stages' host tables, in the order of their dependencies: the k_pyr_group tables read the finished resize tables, the pair
    // records of k_fast2 the finished cells
    std::vector<int16_t> tabs;
    std::vector<CellRec> cells;
    std::vector<uint8_t> pairs;         // empty: this geometry has no pair form
    size_t tree_tab_bytes;              // per (level, image); 0: the quadtree's node tables live in LDS
    int rc;
    orbx_pyramid_plan(e, G, tabs);
    orbx_fast_plan(e, G, cells, pairs);
    if ((rc = orbx_tree_plan(G, &tree_tab_bytes))) return rc;
    ORBX_HIP(orbx_use_device(e->device));
    {   // earlier launches (possibly on a caller's non-blocking stream) still read d_geom / d_tabs / d_cells and the workspaces
        const int qrc = orbx_quiesce(e);
        if (qrc) return qrc;
    }
    const size_t B = e->max_batch;
    // k_desc addresses an image's count row and staging slots with 32-bit byte offsets and multiplies image * pyramid bytes as 32 x 32 bits
    if ((long long)(G.kp_total > ORBX_MAX_LEVELS ? G.kp_total : ORBX_MAX_LEVELS) * (long long)B > (1ll << 30) || G.pyr_bytes >= (1ll << 32)) {
        orbx_set_error("%dx%d with %d staging slots per image and batches of %d: beyond the descriptor stage's 32-bit offsets", w, h, G.kp_total, e->max_batch);
        return ORBX_E_INVALID;
    }
    if ((rc = ensure(&e->d_tabs, &e->tabs_cap, tabs.size() * 2))) return rc;
    if ((rc = ensure(&e->d_cells, &e->cells_cap, cells.size() * sizeof(CellRec)))) return rc;
    if (!pairs.empty() && (rc = ensure(&e->d_pairs, &e->pairs_cap, pairs.size()))) return rc;
    if ((rc = ensure(&e->d_pyr, &e->pyr_cap, (size_t)G.pyr_bytes * B))) return rc;
    if ((rc = ensure(&e->d_cell_cnt, &e->cell_cnt_cap, (size_t)G.total_cells * B * 4))) return rc;
    if ((rc = ensure(&e->d_cand, &e->cand_cap, (size_t)G.cand_total * B * 4))) return rc;
    if ((rc = ensure(&e->d_cand_prim, &e->cand_prim_cap, (size_t)G.total_cells * B * ORBX_CAND_PRIM * 4))) return rc;
    if ((rc = ensure(&e->d_tree_pts, &e->tree_pts_cap, (size_t)G.cand_total * B * 4))) return rc;
    if ((rc = ensure(&e->d_tree_nid, &e->tree_nid_cap, (size_t)G.cand_total * B * 2))) return rc;
    if ((rc = ensure(&e->d_lvl_kp, &e->lvl_kp_cap, (size_t)G.kp_total * B * 4))) return rc;
    if (tree_tab_bytes && (rc = ensure(&e->d_tree_tab, &e->tree_tab_cap, align_up(tree_tab_bytes, 256) * e->nlevels * B))) return rc;
    e->rt_kps = nullptr;
    if (orbx_desc_rowtab_plan(G)) {
        // row table by-product of k_desc: one 16-byte entry per keypoint (orbx_stereo.hip)
        e->rt_ent_cap = G.kp_total;
        if ((rc = ensure(&e->d_rt_off, &e->rt_off_cap, (size_t)(G.lv[0].h + 1) * B * sizeof(int)))) return rc;
        if ((rc = ensure(&e->d_rt_entries, &e->rt_entries_cap, (size_t)e->rt_ent_cap * B * 16))) return rc;
    } else if (e->d_rt_off) {
        ORBX_HIP(hipFree(e->d_rt_off)); e->d_rt_off = nullptr; e->rt_off_cap = 0;
    }
    ORBX_HIP(hipMemcpy(e->d_tabs, tabs.data(), tabs.size() * 2, hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(e->d_cells, cells.data(), cells.size() * sizeof(CellRec), hipMemcpyHostToDevice));
    if (!pairs.empty()) ORBX_HIP(hipMemcpy(e->d_pairs, pairs.data(), pairs.size(), hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(e->d_geom, &G, sizeof G, hipMemcpyHostToDevice));
    if ((rc = orbx_tree_commit(G))) return rc;
    e->geom = G;
    return ORBX_OK;
}

extern "C" int orbx_extractor_set_pyramid_group_limit(orbx_extractor *e, int max_images)
{
    if (!e || max_images < 0) { orbx_set_error("orbx_extractor_set_pyramid_group_limit: invalid argument"); return ORBX_E_INVALID; }
    e->pyr_group_max_images = max_images;       // a launch constant of later extractions; results do not depend on it
    e->pyr_group_mid_images = max_images == 0 ? 0 : e->pyr_group_mid_cfg;       // 0 = one launch per level, always; any other limit: the configured mid size again
    for (orbx_extractor *x : e->lanes) if (x) { x->pyr_group_max_images = max_images; x->pyr_group_mid_images = e->pyr_group_mid_images; }
    return ORBX_OK;
}

extern "C" int orbx_extractor_create(orbx_extractor **out, int nfeatures, float scale_factor, int nlevels,
                                     int ini_th, int min_th, int device, int max_w, int max_h, int max_batch)
{
    if (!out) { orbx_set_error("out is NULL"); return ORBX_E_INVALID; }
    *out = nullptr;
    if (nfeatures < 1 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f) || max_batch < 1 ||
        max_w < 1 || max_h < 1 || ini_th < 1 || min_th < 1 || ini_th > 255 || min_th > ini_th) {
        orbx_set_error("orbx_extractor_create: invalid parameter");
        return ORBX_E_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
        orbx_set_error("no usable HIP device (requested %d of %d); liborbx has no CPU fallback", device, ndev);
        return ORBX_E_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    orbx_extractor *e = new orbx_extractor();
    e->prof_mask = ~0u;
    orbx_extractor_set_cv_profile(e, ORBX_CV_PROFILE_3_2);   // the OpenCV the reference was tested with (README.md:68)
    e->device = device; e->nfeatures = nfeatures; e->nlevels = nlevels; e->ini_th = ini_th; e->min_th = min_th;
    e->scale_factor = scale_factor; e->max_w = max_w; e->max_h = max_h; e->max_batch = max_batch;
    {   // launches of up to this many images build the pyramid with k_pyr_group (2 launches instead of 7); more: k_resize per level
        const char *env = getenv("ORBX_PYR_GROUP_MAX_IMAGES");
        e->pyr_group_max_images = env && *env ? atoi(env) : 8;
        const char *mid = getenv("ORBX_PYR_GROUP_MID_IMAGES");
        e->pyr_group_mid_images = e->pyr_group_mid_cfg = mid && *mid ? atoi(mid) : 24;     // (8 frames: 57.2 -> 59.8 k frames/s; 16 frames: the same; 32: slower)
        const char *kpw = getenv("ORBX_STEREO_KPW");      // tests: k_stereo's one / four keypoints per wave on the same input
        e->stereo_kpw_forced = kpw && (*kpw == '1' || *kpw == '4') ? *kpw - '0' : 0;
        const char *pl = getenv("ORBX_PIPE_LANES"), *pi = getenv("ORBX_PIPE_INLINE");
        // defaults (examples/stereo_stream on one camera stream): four lanes, transport by copy kernel on the lane's stream: 19 k frames/s;
        // copy engines on two copy streams: 15 k whatever the lanes; ORBX_PIPE_INLINE=0 / ORBX_PIPE_KCOPY=0 select the older forms
        e->pipe_lanes = pl && *pl >= '1' && *pl <= '0' + ORBX_PIPE_DEPTH ? *pl - '0' : ORBX_PIPE_DEPTH;
        e->pipe_inline = !(pi && *pi == '0');
        const char *pk = getenv("ORBX_PIPE_KCOPY");
        e->pipe_kcopy = !(pk && *pk == '0');
        // RGB-D depth transport of the pipelined form: gather by default (one stream, 4 in flight: 28.9 k frames/s against 20.4 k with the
        // upload, profiles/r05_rgbd.txt); ORBX_PIPE_RGBD_GATHER=0 uploads the whole depth map into the slot
        const char *pg = getenv("ORBX_PIPE_RGBD_GATHER");
        e->pipe_rgbd_gather = !(pg && *pg == '0');
        const char *fw = getenv("ORBX_FAST_WAVES");      // tests / experiments: force k_fast's waves per cell
        e->fast_waves = fw && *fw >= '1' && *fw <= '4' ? *fw - '0' : 0;
        // ORBX_FAST_PAIR=1: the pair kernel (k_fast2) where the geometry allows.  Off by default: bit-exact, 4 % fewer VALU instructions per cell and
        // less halo traffic, but 5-10 % SLOWER than one cell per wave on MI355X (the kernel sits at the knee between VALU issue
        // and latency, and a pair wave's 7.8 KB of LDS leaves 21 waves per CU against 28)
        const char *fp = getenv("ORBX_FAST_PAIR");
        e->fast_pair = fp && *fp == '1' ? 1 : 0;
        const char *dv = getenv("ORBX_DESC_VALU_ROWPASS");  // tests / A-B: k_desc's older row pass (v_dot4_u32_u8) instead of the matrix cores; same results
        e->desc_valu_rowpass = dv && *dv == '1' ? 1 : 0;
    }
    // src/ORBextractor.cc:436-461
    e->sf[0] = 1.0f; e->sig2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) { e->sf[i] = (float)(e->sf[i - 1] * e->scale_factor); e->sig2[i] = e->sf[i] * e->sf[i]; }
    for (int i = 0; i < nlevels; i++) { e->isf[i] = 1.0f / e->sf[i]; e->isig2[i] = 1.0f / e->sig2[i]; }
    // :468-493
    float factor = (float)(1.0f / e->scale_factor);
    float n_desired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) { e->quota[l] = orbx_cv_round(n_desired); sum += e->quota[l]; n_desired *= factor; }
    e->quota[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
    // :510-533
    {
        int v, v0, vmax = (int)floor(15 * sqrtf(2.f) / 2 + 1), vmin = (int)ceil(15 * sqrtf(2.f) / 2);
        const double hp2 = 15 * 15;
        for (v = 0; v <= vmax; ++v) e->umax[v] = (int)lrint(sqrt(hp2 - v * v));
        for (v = 15, v0 = 0; v >= vmin; --v) { while (e->umax[v0] == e->umax[v0 + 1]) ++v0; e->umax[v] = v0; ++v0; }
    }
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { orbx_set_error("hipStreamCreate failed: %s", hipGetErrorString(he)); delete e; return ORBX_E_HIP; }
    int rc = orbx_desc_upload_constants(e);
    if (rc == ORBX_OK && hipMalloc((void **)&e->d_geom, sizeof(Geom)) != hipSuccess) { orbx_set_error("hipMalloc failed"); rc = ORBX_E_HIP; }
    if (rc == ORBX_OK && hipMalloc((void **)&e->d_lvl_cnt, sizeof(int) * (size_t)max_batch * ORBX_MAX_LEVELS + 16) != hipSuccess) { orbx_set_error("hipMalloc failed"); rc = ORBX_E_HIP; }
    if (rc == ORBX_OK && hipHostMalloc((void **)&e->h_flag, 64, hipHostMallocDefault) != hipSuccess) { orbx_set_error("hipHostMalloc failed"); rc = ORBX_E_HIP; }
    if (rc != ORBX_OK) { orbx_extractor_destroy(e); return rc; }
    *e->h_flag = 0;
    // last int of d_lvl_cnt is the kernel error flag
    hipMemset(e->d_lvl_cnt, 0, sizeof(int) * (size_t)max_batch * ORBX_MAX_LEVELS + 16);
    *out = e;
    return ORBX_OK;
}

extern "C" void orbx_debug_pipe_prof_print();     // orbx_hostapi.hip
extern "C" void orbx_extractor_destroy(orbx_extractor *e)
{
    if (!e) return;
    hipSetDevice(e->device);
    if (e->pipe_counted) orbx_debug_pipe_prof_print();
    for (orbx_extractor *&x : e->lanes) if (x) { orbx_extractor_destroy(x); x = nullptr; }
    if (e->pipe_counted) orbx_pipe_handle_released();
    if (e->stream) hipStreamSynchronize(e->stream);
    for (auto &ev : e->prof_ev) { if (ev.owns_a && ev.a) hipEventDestroy(ev.a); if (ev.b) hipEventDestroy(ev.b); }
    for (auto ev : e->prof_pool) hipEventDestroy(ev);
    if (e->ev_switch) hipEventDestroy(e->ev_switch);
    void *ptrs[] = { e->d_cand_prim, e->d_tree_tab, e->d_cells, e->d_pairs, e->d_geom, e->d_tabs, e->d_pyr, e->d_stage_in, e->d_cell_cnt, e->d_cand, e->d_tree_pts, e->d_tree_nid,
                     e->d_lvl_cnt, e->d_lvl_kp, e->d_out_kps, e->d_out_desc, e->d_out_n, e->d_out_ur, e->d_out_depth, e->d_st_dist, e->d_st_entries, e->d_rt_off, e->d_rt_entries, e->d_st_arrive };
    for (void *p : ptrs) if (p) hipFree(p);
    for (void *p : e->scratch) if (p) hipFree(p);
    for (PipeSlot &s : e->pipe) {
        if (s.ev_d2h) hipEventSynchronize(s.ev_d2h);
        void *dp[] = { s.d_in, s.d_out };
        for (void *p : dp) if (p) hipFree(p);
        if (s.h_in) hipHostFree(s.h_in);
        if (s.h_out) hipHostFree(s.h_out);
        hipEvent_t evs[] = { s.ev_h2d, s.ev_done, s.ev_d2h };
        for (hipEvent_t ev : evs) if (ev) hipEventDestroy(ev);
    }
    if (e->copy_in) hipStreamDestroy(e->copy_in);
    if (e->copy_out) hipStreamDestroy(e->copy_out);
    if (e->h_stage_in) hipHostFree(e->h_stage_in);
    if (e->h_out) hipHostFree(e->h_out);
    if (e->h_flag) hipHostFree(e->h_flag);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

extern "C" int orbx_get_levels(const orbx_extractor *e) { return e ? e->nlevels : ORBX_E_INVALID; }
extern "C" float orbx_get_scale_factor(const orbx_extractor *e) { return e ? (float)e->scale_factor : 0.f; }
extern "C" int orbx_get_scale_tables(const orbx_extractor *e, float *s, float *is, float *g2, float *ig2)
{
    if (!e) { orbx_set_error("null extractor"); return ORBX_E_INVALID; }
    for (int i = 0; i < e->nlevels; i++) {
        if (s) s[i] = e->sf[i];
        if (is) is[i] = e->isf[i];
        if (g2) g2[i] = e->sig2[i];
        if (ig2) ig2[i] = e->isig2[i];
    }
    return ORBX_OK;
}
extern "C" int orbx_get_features_per_level(const orbx_extractor *e, int *q)
{
    if (!e || !q) { orbx_set_error("null argument"); return ORBX_E_INVALID; }
    for (int i = 0; i < e->nlevels; i++) q[i] = e->quota[i];
    return ORBX_OK;
}

extern "C" int orbx_max_keypoints(const orbx_extractor *e, int w, int h)
{
    if (!e || w < 1 || h < 1) { orbx_set_error("invalid argument"); return ORBX_E_INVALID; }
    int total = 0;
    for (int l = 0; l < e->nlevels; l++) {
        const int lw = orbx_cv_round((float)w * e->isf[l]), lh = orbx_cv_round((float)h * e->isf[l]);
        const int tw = lw - 32, th = lh - 32;
        if (tw < 30 || th < 30) { orbx_set_error("image too small"); return ORBX_E_TOO_SMALL; }
        const int n_ini = (int)roundf((float)tw / th);
        const int nc = e->quota[l] + 3 > 4 * n_ini ? e->quota[l] + 3 : 4 * n_ini;
        total += (nc + 4 + 3) & ~3;
    }
    return total;
}

int orbx_use_stream(orbx_extractor *e, hipStream_t s)
{
    if (e->last_launch_stream && e->last_launch_stream != s) {
        if (!e->ev_switch) ORBX_HIP(hipEventCreateWithFlags(&e->ev_switch, hipEventDisableTiming));
        ORBX_HIP(hipEventRecord(e->ev_switch, e->last_launch_stream));
        ORBX_HIP(hipStreamWaitEvent(s, e->ev_switch, 0));
    }
    e->last_launch_stream = s;
    return ORBX_OK;
}

extern "C" int orbx_extract_batch_device(orbx_extractor *e, const void *d_imgs, size_t img_stride, size_t pitch,
                                         int batch, int w, int h, void *d_kps, void *d_desc, int cap, void *d_n_out,
                                         void *stream)
{
    if (!e || !d_imgs || !d_kps || !d_desc || !d_n_out || batch < 1 || batch > e->max_batch || w < 1 || h < 1 ||
        pitch < (size_t)w || (batch > 1 && img_stride < pitch * (size_t)h)) {
        orbx_set_error("orbx_extract_batch_device: invalid argument");
        return ORBX_E_INVALID;
    }
    ORBX_HIP(orbx_use_device(e->device));
    int rc = orbx_prepare_geometry(e, w, h);
    if (rc) return rc;
    const Geom &G = e->geom;
    if (cap < G.kp_total) {
        orbx_set_error("keypoint capacity %d < orbx_max_keypoints() = %d", cap, G.kp_total);
        return ORBX_E_CAPACITY;
    }
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    if ((rc = orbx_use_stream(e, s))) return rc;
    PyrRef pr;
    pr.img0 = (const uint8_t *)d_imgs; pr.img0_stride = (long long)img_stride; pr.img0_pitch = (int)pitch;
    pr.pyr = e->d_pyr; pr.pyr_stride = G.pyr_bytes;
    e->last_img0 = pr.img0; e->last_img_stride = img_stride; e->last_pitch = pitch; e->last_batch = batch;

    // each stage launches from its own file and notes the form it took in e->last_forms (orbx_debug_launch_forms; stereo fields: orbx_stereo.hip)
    orbx_pyramid_launch(e, pr, batch, s);       // (an ORBX_STAGE_RESIZE pair around every launch of its chain)
    orbx_prof_begin(e, ORBX_STAGE_FAST, s);
    orbx_fast_launch(e, pr, batch, s);
    orbx_prof_end(e, s);
    orbx_prof_begin(e, ORBX_STAGE_TREE, s);
    orbx_tree_launch(e, batch, s);
    orbx_prof_end(e, s);
    orbx_prof_begin(e, ORBX_STAGE_DESC, s);
    orbx_desc_launch(e, pr, batch, d_kps, d_desc, d_n_out, cap, s);
    orbx_prof_end(e, s);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_sync(orbx_extractor *e, void *stream)
{
    if (!e) { orbx_set_error("null extractor"); return ORBX_E_INVALID; }
    ORBX_HIP(orbx_use_device(e->device));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    // the kernel error flag rides the same stream into pinned memory: one synchronisation, no blocking pageable copy
    int *d_flag = orbx_err_flag(e);
    ORBX_HIP(hipMemcpyAsync(e->h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    ORBX_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), s)); // the error belongs to the work synchronised here, not to later frames
    ORBX_HIP(hipStreamSynchronize(s));
    e->prof_chain = false; // the stream idles from here on: the next launch must not share its begin event with the last one
    const int flag = *e->h_flag;
    if (flag) { orbx_set_error("quadtree kernel reported a node-table overflow"); return ORBX_E_CAPACITY; }
    return ORBX_OK;
}

int orbx_quiesce(orbx_extractor *e)
{
    for (orbx_extractor *x : e->lanes) if (x) { const int lrc = orbx_quiesce(x); if (lrc) return lrc; }
    ORBX_HIP(hipStreamSynchronize(e->stream));
    if (e->last_launch_stream && e->last_launch_stream != e->stream) ORBX_HIP(hipStreamSynchronize(e->last_launch_stream));
    if (e->copy_in) ORBX_HIP(hipStreamSynchronize(e->copy_in));
    if (e->copy_out) ORBX_HIP(hipStreamSynchronize(e->copy_out));
    return ORBX_OK;
}

extern "C" int orbx_pyramid_level(orbx_extractor *e, int image_index, int level, uint8_t *dst, size_t dst_stride, int *w, int *h)
{
    if (!e || !e->geom.w || !e->last_img0 || level < 0 || level >= e->nlevels || image_index < 0 || image_index >= e->last_batch) {
        orbx_set_error("orbx_pyramid_level: no pyramid / bad index");
        return ORBX_E_INVALID;
    }
    const LevelGeom &L = e->geom.lv[level];
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (!dst) return ORBX_OK;
    if (dst_stride < (size_t)L.w) { orbx_set_error("dst_stride < level width"); return ORBX_E_INVALID; }
    ORBX_HIP(orbx_use_device(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    const uint8_t *src; size_t pitch;
    if (level == 0) { src = e->last_img0 + e->last_img_stride * image_index; pitch = e->last_pitch; }
    else { src = e->d_pyr + (size_t)e->geom.pyr_bytes * image_index + L.pyr_off; pitch = L.pitch; }
    ORBX_HIP(hipMemcpy2D(dst, dst_stride, src, pitch, L.w, L.h, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// which FAST kernel the most recent extraction launched: 1 = k_fast (a cell per wave, or several waves per cell), 2 = k_fast2 (a pair of cells per wave)
extern "C" int orbx_debug_fast_form(const orbx_extractor *e) { return e ? e->last_fast_form : ORBX_E_INVALID; }

extern "C" int orbx_debug_launch_forms(const orbx_extractor *e, int32_t *out, int n)
{
    if (!e || n < 0 || (n > 0 && !out)) { orbx_set_error("orbx_debug_launch_forms: invalid argument"); return ORBX_E_INVALID; }
    for (int i = 0; i < n && i < ORBX_LAUNCH_FORM_FIELDS; i++) out[i] = e->last_forms[i];
    return ORBX_LAUNCH_FORM_FIELDS;
}

extern "C" int orbx_debug_level_counts(orbx_extractor *e, int image_index, int32_t *counts)
{
    if (!e || !counts || image_index < 0 || image_index >= e->last_batch) { orbx_set_error("bad argument"); return ORBX_E_INVALID; }
    ORBX_HIP(orbx_use_device(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    ORBX_HIP(hipMemcpy(counts, e->d_lvl_cnt + (size_t)image_index * ORBX_MAX_LEVELS, sizeof(int) * e->nlevels, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_debug_candidates(orbx_extractor *e, int image_index, int level, int32_t *x, int32_t *y, int32_t *resp, int cap, int *n)
{
    if (!e || !n || !e->geom.w || level < 0 || level >= e->nlevels || image_index < 0 || image_index >= e->last_batch) {
        orbx_set_error("bad argument");
        return ORBX_E_INVALID;
    }
    ORBX_HIP(orbx_use_device(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    const Geom &G = e->geom;
    const LevelGeom &L = G.lv[level];
    std::vector<int> cnt(L.n_cells);
    std::vector<uint32_t> slots((size_t)L.n_cells * L.cand_cap);
    ORBX_HIP(hipMemcpy(cnt.data(), e->d_cell_cnt + (size_t)image_index * G.total_cells + L.cell_base, sizeof(int) * L.n_cells, hipMemcpyDeviceToHost));
    ORBX_HIP(hipMemcpy(slots.data(), e->d_cand + (size_t)image_index * G.cand_total + L.cand_off, slots.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> prim((size_t)L.n_cells * ORBX_CAND_PRIM);
    ORBX_HIP(hipMemcpy(prim.data(), e->d_cand_prim + ((size_t)image_index * G.total_cells + L.cell_base) * ORBX_CAND_PRIM, prim.size() * 4, hipMemcpyDeviceToHost));
    int k = 0;
    for (int c = 0; c < L.n_cells; c++)
        for (int i = 0; i < cnt[c]; i++, k++)
            if (k < cap && x && y && resp) {
                const uint32_t p = i < ORBX_CAND_PRIM ? prim[(size_t)c * ORBX_CAND_PRIM + i] : slots[(size_t)c * L.cand_cap + i];
                x[k] = p & 0xFFF; y[k] = (p >> 12) & 0xFFF; resp[k] = p >> 24;
            }
    *n = k;
    return ORBX_OK;
}

int orbx_scratch(orbx_extractor *e, int slot, size_t bytes, void **out)
{
    if (bytes > e->scratch_cap[slot] || !e->scratch[slot]) {
        { const int qrc = orbx_quiesce(e); if (qrc) return qrc; }
        { const int rc = ensure(&e->scratch[slot], &e->scratch_cap[slot], bytes); if (rc) return rc; }
    }
    *out = e->scratch[slot];
    return ORBX_OK;
}

#ifdef ORBX_DIAG
extern "C" int orbx_diag_spans(unsigned *out /*[2][SPAN_SLOTS][2]*/, int reset)
{
    ORBX_HIP(hipDeviceSynchronize());
    const int rc = orbx_fast_diag_spans(out, reset);
    return rc ? rc : orbx_desc_diag_spans(out + 2 * SPAN_SLOTS, reset);
}
#endif
