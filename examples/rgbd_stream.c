/* A host-fed RGB-D camera stream through the pipelined C ABI: the frame loop of the reference's Examples/RGB-D/rgbd_tum.cc:77-119
 * (imread colour + 16-bit depth, SLAM.TrackRGBD -> Tracking::GrabImageRGBD -> Frame::Frame(imGray, imDepth, ...)) with the per-frame
 * work up to ComputeStereoFromRGBD behind orbx_extract_rgbd_submit / orbx_extract_rgbd_wait.  One handle, TUM1 settings
 * (Examples/RGB-D/TUM1.yaml), 640 x 480 frames of a synthetic texture and a synthetic uint16 depth map.  Runs the stream with 1 and with 4
 * frames in flight and prints one JSON line: frames/s and p50 / p99 submit -> wait latency of each.
 *   gcc -O2 -std=c99 -Iinclude examples/rgbd_stream.c -Lorb-slam2_amd -lorbx -Wl,-rpath,$PWD/orb-slam2_amd -o rgbd_stream
 *   ./rgbd_stream [--frames N] [--channels 1|3|4] [--pageable]
 * ORBX_PIPE_RGBD_GATHER=0 selects the upload transport of the depth map instead of the default gather (include/orbx.h). */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "orbx.h"

#define W 640
#define H 480
#define NIMG 4

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static int cmp_float(const void *a, const void *b) { const float x = *(const float *)a, y = *(const float *)b; return x < y ? -1 : x > y; }

/* one timed stream of `frames` frames with `depth` in flight; latency of each frame from its submit to its wait returning */
static int run(orbx_extractor *ex, uint8_t **img, uint16_t **dep, int ch, const orbx_rgbd_params *p, int frames, int depth,
               double *fps, double *p50, double *p99, long *valid)
{
    const int cap = orbx_max_keypoints(ex, W, H);
    orbx_keypoint *kps = (orbx_keypoint *)malloc(sizeof(orbx_keypoint) * (size_t)cap);
    uint8_t *desc = (uint8_t *)malloc((size_t)32 * cap);
    float *ur = (float *)malloc(4 * (size_t)cap), *z = (float *)malloc(4 * (size_t)cap), *lat = (float *)malloc(sizeof(float) * (size_t)frames);
    int tickets[8], n = 0, rc = 0, nl = 0;
    double t_sub[8];
    *valid = 0;
    const double t0 = now();
    for (int i = 0; i < frames + depth && !rc; i++) {
        if (i >= depth) {
            const int s = (i - depth) % depth;
            rc = orbx_extract_rgbd_wait(ex, tickets[s], kps, desc, cap, &n, NULL, ur, z);
            lat[nl++] = (float)(1e6 * (now() - t_sub[s]));
            for (int k = 0; k < n && !rc; k++) *valid += z[k] > 0;
        }
        if (i < frames && !rc) {
            const int s = i % depth;
            t_sub[s] = now();
            rc = orbx_extract_rgbd_submit(ex, img[i % NIMG], W, H, (size_t)W * ch, ch, 1, dep[i % NIMG], (size_t)W * 2, p, &tickets[s]);
        }
    }
    const double el = now() - t0;
    if (rc) fprintf(stderr, "stream: %s\n", orbx_last_error());
    qsort(lat, (size_t)nl, sizeof(float), cmp_float);
    *fps = frames / el;
    *p50 = nl ? lat[nl / 2] : 0;
    *p99 = nl ? lat[(int)(0.99 * (nl - 1))] : 0;
    free(kps); free(desc); free(ur); free(z); free(lat);
    return rc;
}

int main(int argc, char **argv)
{
    int frames = 1000, ch = 3, pinned = 1;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--frames") && i + 1 < argc) frames = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--channels") && i + 1 < argc) ch = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--pageable")) pinned = 0;
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 1; }
    }
    if (frames < 1 || (ch != 1 && ch != 3 && ch != 4) || orbx_device_count() < 1) { fprintf(stderr, "no device / bad arguments\n"); return 2; }
    /* Examples/RGB-D/TUM1.yaml; Tracking::mDepthMapFactor = 1.0f / DepthMapFactor (src/Tracking.cc:147-151) */
    orbx_rgbd_params p;
    memset(&p, 0, sizeof p);
    p.depth_type = ORBX_DEPTH_U16; p.depth_scale = 1.0f / 5000.0f; p.bf = 40.0f;
    p.fx = 517.306408f; p.fy = 516.469215f; p.cx = 318.643040f; p.cy = 255.313989f;
    const float dist[5] = { 0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f };
    memcpy(p.dist_coef, dist, sizeof dist); p.ndist = 5;
    uint8_t *img[NIMG]; uint16_t *dep[NIMG];
    for (int k = 0; k < NIMG; k++) {
        const size_t ib = (size_t)W * H * ch, db = (size_t)W * H * 2;
        img[k] = pinned ? (uint8_t *)orbx_pinned_alloc(ib) : (uint8_t *)malloc(ib);
        dep[k] = pinned ? (uint16_t *)orbx_pinned_alloc(db) : (uint16_t *)malloc(db);
        if (!img[k] || !dep[k]) { fprintf(stderr, "allocation failed\n"); return 2; }
        unsigned s = 777u + 31u * k;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                s = s * 1664525u + 1013904223u;
                for (int c = 0; c < ch; c++) img[k][((size_t)y * W + x) * ch + c] = (uint8_t)(((x / 20) * 37 + (y / 20) * 91 + 29 * c + 13 * k) % 200 + (s >> 28));
                dep[k][(size_t)y * W + x] = (s >> 24) < 16 ? 0 : (uint16_t)(4000 + 20 * x + 7 * y);   /* ~6 % holes, 0.8 - 3.6 m */
            }
    }
    orbx_extractor *ex = NULL;
    if (orbx_extractor_create(&ex, 1000, 1.2f, 8, 20, 7, 0, W, H, 2)) { fprintf(stderr, "create: %s\n", orbx_last_error()); return 2; }
    double fps[2], p50[2], p99[2];
    long valid[2];
    int rc = 0;
    const int depths[2] = { 1, orbx_pipeline_depth() };
    for (int r = 0; r < 2 && !rc; r++) {
        double a, b, c; long v;
        rc = run(ex, img, dep, ch, &p, depths[r] * 8, depths[r], &a, &b, &c, &v);          /* warm-up outside the timed run */
        if (!rc) rc = run(ex, img, dep, ch, &p, frames, depths[r], &fps[r], &p50[r], &p99[r], &valid[r]);
    }
    orbx_extractor_destroy(ex);
    if (rc) return 3;
    printf("{\"w\": %d, \"h\": %d, \"channels\": %d, \"pinned\": %s, \"frames\": %d, \"depth_transport\": \"%s\", "
           "\"in_flight_1\": {\"frames_per_s\": %.1f, \"latency_us_p50\": %.1f, \"latency_us_p99\": %.1f}, "
           "\"in_flight_%d\": {\"frames_per_s\": %.1f, \"latency_us_p50\": %.1f, \"latency_us_p99\": %.1f}, \"valid_depth_per_frame\": %.1f}\n",
           W, H, ch, pinned ? "true" : "false", frames, getenv("ORBX_PIPE_RGBD_GATHER") && *getenv("ORBX_PIPE_RGBD_GATHER") == '0' ? "upload" : "gather",
           fps[0], p50[0], p99[0], depths[1], fps[1], p50[1], p99[1], (double)valid[1] / frames);
    return 0;
}
