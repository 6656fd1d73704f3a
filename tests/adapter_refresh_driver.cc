// Driver of adapter/mappoint/MapPointRefresh.cc (tests/test_refresh_adapter.py): a stub map built through the stand-in mutators of
// tests/cvstub_refresh, whose keyframes lie in ONE array in the order they are made -- so the order of their addresses, in which the
// reference walks a point's observations, is the order of their slots, in which the device call does.  orbx_adapter::RefreshMapPoints must
// then leave every MapPoint member byte-equal (NaN equal to NaN) to MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors run point by
// point: with and without a map-point table, with bad keyframes whose observations linger, with a reference keyframe outside the row,
// with a point the graph does not know, and with the descriptors on the host while a keyframe has no resident frame.  The table is the
// real orbx_adapter::LocalMapPoints (adapter/localmap/LocalMapPoints.cc) behind the hooks it announces itself with: a SearchLocalPoints
// fills it, the members change on the host, RefreshMapPoints writes it in place, and the next SearchLocalPoints must find nothing to send
// while every slot holds its point's members.
//   adapter_refresh_driver check
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <map>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Frame.h"
#include "MapGraph.h"
#include "LocalMapPoints.h"
#include "orbx_adapter.h"
#include "MapPointRefresh.h"
#include "orbx_device.h"

namespace ORB_SLAM2 { bool g_hooks = false; }
using namespace ORB_SLAM2;
using std::vector;

static unsigned g_rng = 12345u;
static unsigned rnd(unsigned n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 16) / 65536.f; }

#define NKF 12
#define NFEAT 30
#define NPT 160
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static KeyFrame *g_kf;                                   // NKF keyframes in one array
static vector<MapPoint *> g_pt;
static std::map<KeyFrame *, std::shared_ptr<const orbx_frame> > g_frames;
static std::shared_ptr<const orbx_frame> frame_of(KeyFrame *pKF)
{
    std::map<KeyFrame *, std::shared_ptr<const orbx_frame> >::iterator it = g_frames.find(pKF);
    return it == g_frames.end() ? std::shared_ptr<const orbx_frame>() : it->second;
}
namespace ORB_SLAM2 {
float Frame::fx = 500.f, Frame::fy = 500.f, Frame::cx = 320.f, Frame::cy = 240.f;
float Frame::mnMinX = 0.f, Frame::mnMaxX = 640.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 480.f;
}
// LocalMapPoints.cc asks for the frame's resident copy (adapter/ORBmatcher_proj.cc in a full build): the driver's one frame
static orbx_frame *g_resident;
namespace orbx_adapter { orbx_frame *ResidentFrame(const ORB_SLAM2::Frame &) { return g_resident; } }

static void destroy_frame(const orbx_frame *f) { orbx_frame_destroy(const_cast<orbx_frame *>(f)); }

static int make_frame(KeyFrame *pKF)
{
    const int n = pKF->N;
    vector<float> x(n, 10.f), y(n, 10.f), angle(n, 0.f), ur(n, -1.f);
    vector<int32_t> oct(n);
    for (int i = 0; i < n; i++) oct[i] = pKF->mvKeysUn[i].octave;
    orbx_frame_feats ff;
    memset(&ff, 0, sizeof ff);
    ff.n = n; ff.x = &x[0]; ff.y = &y[0]; ff.octave = &oct[0]; ff.angle = &angle[0]; ff.u_right = &ur[0]; ff.desc = pKF->mDescriptors.data;
    ff.min_x = 0.f; ff.min_y = 0.f; ff.max_x = 640.f; ff.max_y = 480.f;
    orbx_frame *f = NULL;
    if (orbx_frame_create(orbx_adapter::Device(), &ff, &f) != ORBX_OK) { fprintf(stderr, "%s\n", orbx_last_error()); return 1; }
    g_frames[pKF] = std::shared_ptr<const orbx_frame>(f, destroy_frame);
    return 0;
}

struct Members { bool has_normal, has_desc; float normal[3], dmin, dmax; unsigned char desc[32]; };

static Members members(MapPoint *p)
{
    Members m;
    memset(&m, 0, sizeof m);
    m.has_normal = !p->mNormalVector.empty(); m.has_desc = !p->mDescriptor.empty();
    if (m.has_normal) for (int c = 0; c < 3; c++) m.normal[c] = p->mNormalVector.at<float>(c);
    m.dmin = p->mfMinDistance; m.dmax = p->mfMaxDistance;
    if (m.has_desc) memcpy(m.desc, p->mDescriptor.data, 32);
    return m;
}

static bool same_float(float a, float b) { return a != a ? b != b : memcmp(&a, &b, 4) == 0; }     // equal bytes, or both NaN
static bool same(const Members &a, const Members &b)
{
    bool ok = a.has_normal == b.has_normal && a.has_desc == b.has_desc && same_float(a.dmin, b.dmin) && same_float(a.dmax, b.dmax);
    for (int c = 0; c < 3; c++) ok = ok && same_float(a.normal[c], b.normal[c]);
    return ok && memcmp(a.desc, b.desc, 32) == 0;
}

// members that neither route has written yet
static void scrub(MapPoint *p)
{
    p->mNormalVector = cv::Mat(); p->mDescriptor = cv::Mat(); p->mfMinDistance = -7.f; p->mfMaxDistance = -7.f;
}

// one comparison: the adaptor over `list`, then the reference's functions over the same points
static int compare(const char *tag, const vector<MapPoint *> &list, int what, orbx_adapter::RefreshStats *st)
{
    for (size_t i = 0; i < g_pt.size(); i++) scrub(g_pt[i]);
    *st = orbx_adapter::RefreshMapPoints(list, what);
    vector<Members> got(g_pt.size());
    for (size_t i = 0; i < g_pt.size(); i++) got[i] = members(g_pt[i]);
    for (size_t i = 0; i < g_pt.size(); i++) scrub(g_pt[i]);
    std::map<MapPoint *, int> once;
    for (size_t i = 0; i < list.size(); i++) {
        if (!list[i] || once[list[i]]++) continue;
        if (what & 1) list[i]->UpdateNormalAndDepth();
        if (what & 2) list[i]->ComputeDistinctiveDescriptors();
    }
    int updated = 0;
    for (size_t i = 0; i < g_pt.size(); i++) {
        const Members want = members(g_pt[i]);
        if (!same(want, got[i]))
            FAIL("%s: point %zu differs: normal %d/%d (%.9g %.9g %.9g | %.9g %.9g %.9g) min %.9g | %.9g max %.9g | %.9g desc %d/%d first byte %d | %d", tag, i,
                 (int)got[i].has_normal, (int)want.has_normal, got[i].normal[0], got[i].normal[1], got[i].normal[2], want.normal[0], want.normal[1],
                 want.normal[2], got[i].dmin, want.dmin, got[i].dmax, want.dmax, (int)got[i].has_desc, (int)want.has_desc, got[i].desc[0], want.desc[0]);
        updated += want.has_normal || want.has_desc;
    }
    printf("%s: %d points updated, %d on the device, %d on the host, descriptors of %d on the host, %d ABI calls\n", tag, updated, st->on_device,
           st->on_host, st->desc_on_host, st->abi_calls);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "check") != 0) { fprintf(stderr, "usage: adapter_refresh_driver check\n"); return 2; }
    g_hooks = true;
    g_kf = (KeyFrame *)malloc(NKF * sizeof(KeyFrame));
    vector<float> sf(8);
    for (int l = 0; l < 8; l++) sf[l] = l ? sf[l - 1] * 1.2f : 1.f;
    for (int k = 0; k < NKF; k++) {
        vector<int> oct(NFEAT);
        for (int i = 0; i < NFEAT; i++) oct[i] = (int)rnd(8);
        KeyFrame *pKF = new (&g_kf[k]) KeyFrame((unsigned long)k, oct, vector<float>(NFEAT, -1.f), vector<float>(NFEAT, -1.f), 40.f);
        pKF->mvScaleFactors = sf; pKF->mnScaleLevels = 8;
        pKF->mDescriptors = cv::Mat(NFEAT, 32, CV_8U);
        for (int i = 0; i < NFEAT * 32; i++) pKF->mDescriptors.data[i] = (unsigned char)rnd(256);
        for (int c = 0; c < 3; c++) pKF->Ow.at<float>(c) = rndf(-2.f, 2.f) - (c == 2 ? 6.f : 0.f);
    }
    // points: 2 to 9 observers each; most matches follow the observations
    for (int p = 0; p < NPT; p++) {
        MapPoint *pMP = new MapPoint((unsigned long)p);
        for (int c = 0; c < 3; c++) pMP->mWorldPos.at<float>(c) = rndf(-1.5f, 1.5f);
        const int n = 2 + (int)rnd(8);
        for (int t = 0; t < n; t++) {
            KeyFrame *pKF = &g_kf[rnd(NKF)];
            const size_t idx = rnd(NFEAT);
            if (pMP->IsInKeyFrame(pKF)) continue;
            pMP->AddObservation(pKF, idx);
            if (!pMP->mpRefKF) pMP->mpRefKF = pKF;
            if (rnd(10) < 8) pKF->AddMapPoint(pMP, idx);
        }
        g_pt.push_back(pMP);
    }
    // reference keyframes outside the row (feature 0's octave), and a point at a camera centre (0 * inf)
    int outside = 0;
    for (int p = 0; p < NPT && outside < 12; p += 5)
        for (int k = 0; k < NKF; k++)
            if (!g_pt[p]->IsInKeyFrame(&g_kf[k])) { g_pt[p]->mpRefKF = &g_kf[k]; outside++; break; }
    g_pt[7]->mWorldPos = g_pt[7]->mObservations.begin()->first->GetCameraCenter();
    // a point the graph does not know
    g_hooks = false;
    MapPoint *stranger = new MapPoint(9999);
    for (int c = 0; c < 3; c++) stranger->mWorldPos.at<float>(c) = rndf(-1.f, 1.f);
    stranger->AddObservation(&g_kf[1], 3); stranger->AddObservation(&g_kf[4], 8); stranger->AddObservation(&g_kf[9], 2);
    stranger->mpRefKF = &g_kf[4];
    g_hooks = true;
    g_pt.push_back(stranger);

    orbx_adapter::RefreshStats st;
    vector<MapPoint *> all(g_pt);
    all.push_back(NULL); all.push_back(g_pt[3]);        // a hole, and a point listed twice

    // 1. no resident frames registered: the geometry on the device, the descriptors on the host
    if (compare("no frames", all, 3, &st)) return 1;
    if (st.on_device != NPT || st.on_host != 1 || st.desc_on_host != NPT || st.abi_calls != 1) FAIL("no frames: what ran where");

    // 2. every keyframe resident
    orbx_adapter::refresh_hooks().frame_of.store(&frame_of);
    for (int k = 0; k < NKF; k++) if (make_frame(&g_kf[k])) return 1;
    for (int what = 1; what <= 3; what++) {
        if (compare(what == 1 ? "geometry" : what == 2 ? "descriptors" : "both", all, what, &st)) return 1;
        if (st.on_device != NPT || st.on_host != 1 || st.desc_on_host != 0 || st.abi_calls != 1) FAIL("resident: what ran where");
    }

    // 3. two keyframes go bad: their matched points lose the observation (some points go bad with it), observations without a match
    //    linger and count in the normal; a bad keyframe needs no frame
    g_kf[2].SetBadFlag(); g_kf[8].SetBadFlag();
    g_frames.erase(&g_kf[2]); g_frames.erase(&g_kf[8]);
    int lingering = 0, bad_points = 0;
    for (int p = 0; p < NPT; p++) {
        lingering += g_pt[p]->IsInKeyFrame(&g_kf[2]) || g_pt[p]->IsInKeyFrame(&g_kf[8]);
        bad_points += g_pt[p]->isBad();
        if (g_pt[p]->mpRefKF == &g_kf[2] || g_pt[p]->mpRefKF == &g_kf[8]) g_pt[p]->mpRefKF = &g_kf[5];     // a reference keyframe is in use
    }
    if (!lingering || !bad_points) FAIL("the map has %d lingering observations and %d bad points: the scene is too tame", lingering, bad_points);
    if (compare("bad keyframes", all, 3, &st)) return 1;

    // 4. with the process's map-point table.  A frame looks at every second point: SearchLocalPoints makes the table and sends their
    //    records.  Then the members change on the host (compare() scrubs them all), RefreshMapPoints writes the table in place, and
    //    LocalMapPoints must know: the next search sends nothing, and every slot holds what its point's members say.
    Frame F;
    F.N = 40; F.mnId = 1; F.mbf = 40.f;
    F.mvKeysUn.resize(40); F.mvuRight.assign(40, -1.f); F.mvpMapPoints.assign(40, (MapPoint *)NULL);
    F.mDescriptors = cv::Mat(40, 32, CV_8U);
    for (int i = 0; i < 40 * 32; i++) F.mDescriptors.data[i] = (unsigned char)rnd(256);
    for (int i = 0; i < 40; i++) { F.mvKeysUn[i].pt.x = rndf(5.f, 635.f); F.mvKeysUn[i].pt.y = rndf(5.f, 475.f); F.mvKeysUn[i].octave = (int)rnd(8); F.mvKeysUn[i].angle = 0.f; }
    F.mvScaleFactors = sf; F.mnScaleLevels = 8; F.mfLogScaleFactor = logf(1.2f);
    F.mRcw = cv::Mat(3, 3, CV_32F); F.mtcw = cv::Mat(3, 1, CV_32F); F.mOw = cv::Mat(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) F.mRcw.at<float>(c, c) = 1.f;
    F.mtcw.at<float>(2) = 6.f; F.mOw.at<float>(2) = -6.f;
    {
        vector<float> x(40), y(40), angle(40, 0.f), ur(40, -1.f);
        vector<int32_t> oct(40);
        for (int i = 0; i < 40; i++) { x[i] = F.mvKeysUn[i].pt.x; y[i] = F.mvKeysUn[i].pt.y; oct[i] = F.mvKeysUn[i].octave; }
        orbx_frame_feats ff;
        memset(&ff, 0, sizeof ff);
        ff.n = 40; ff.x = &x[0]; ff.y = &y[0]; ff.octave = &oct[0]; ff.angle = &angle[0]; ff.u_right = &ur[0]; ff.desc = F.mDescriptors.data;
        ff.max_x = 640.f; ff.max_y = 480.f;
        if (orbx_frame_create(orbx_adapter::Device(), &ff, &g_resident) != ORBX_OK) FAIL("%s", orbx_last_error());
    }
    orbx_adapter::LocalMapPoints &M = orbx_adapter::LocalMapPoints::instance();
    vector<MapPoint *> local;
    for (int p = 0; p < NPT; p += 2) local.push_back(g_pt[p]);
    int nToMatch = 0, live = 0;
    for (size_t i = 0; i < local.size(); i++) live += !local[i]->isBad();
    orbx_adapter::SearchLocalPoints(F, local, 1.f, nToMatch);
    if (M.last_uploaded() != live || live < 40) FAIL("with the table: the first search sent %d records, %d points are live", M.last_uploaded(), live);
    if (!orbx_adapter::refresh_hooks().table.load()) FAIL("with the table: LocalMapPoints did not announce itself");
    if (compare("with the table", all, 3, &st)) return 1;
    if (st.abi_calls != 2) FAIL("with the table: %d ABI calls", st.abi_calls);
    int in_table = 0;
    orbx_mappoints *table = M.lend();
    if (!table) FAIL("with the table: no table");
    for (size_t i = 0; i < local.size(); i++) {
        MapPoint *pMP = local[i];
        const int32_t slot = M.lent_slot(pMP);
        if (pMP->isBad()) continue;
        float geom[8], want[8];
        unsigned char desc[32], want_desc[32];
        if (slot < 0 || orbx_mappoints_read(table, &slot, 1, geom, desc) != ORBX_OK) { M.give_back(); FAIL("with the table: point %zu has slot %d: %s", i, (int)slot, orbx_last_error()); }
        pMP->GetFrustumRecord(want, want_desc);
        bool ok = memcmp(desc, want_desc, 32) == 0;
        for (int c = 0; c < 8; c++) ok = ok && same_float(geom[c], want[c]);
        if (!ok) { M.give_back(); FAIL("with the table: slot %d does not hold the members of local point %zu", (int)slot, i); }
        in_table++;
    }
    M.give_back();
    F.mnId = 2;
    orbx_adapter::SearchLocalPoints(F, local, 1.f, nToMatch);
    if (M.last_uploaded() != 0) FAIL("with the table: the search behind the refresh sent %d records again", M.last_uploaded());
    // and a change the refresh did not make is still sent
    local[1]->mfMaxDistance *= 2.f;
    F.mnId = 3;
    orbx_adapter::SearchLocalPoints(F, local, 1.f, nToMatch);
    if (M.last_uploaded() != (local[1]->isBad() ? 0 : 1)) FAIL("with the table: a host change sent %d records", M.last_uploaded());
    if (in_table != live) FAIL("with the table: %d records checked, %d live", in_table, live);
    orbx_frame_destroy(g_resident);
    g_frames.clear();
    printf("adaptor refresh ok: %d lingering observations, %d bad points, %d reference keyframes outside the row, %d table records\n", lingering,
           bad_points, outside, in_table);
    return 0;
}
