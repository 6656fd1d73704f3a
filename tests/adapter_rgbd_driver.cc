// tests/adapter_rgbd_driver.cc -- drives ORBextractor::ExtractRGBD (adapter/ORBextractor_rgbd.cc) for tests/test_rgbd.py.
// usage: adapter_rgbd_driver <gray.raw> <depth.raw> <w> <h> <u16|f32> <padded 0|1> <depthScale> <bf> <fx fy cx cy> <ndist> <k...> <out.bin>
// The depth Mat is built by hand (the stub's Mat knows no 16-bit element size): data / step set directly, with `padded` a row step
// larger than a row (a non-continuous Mat, as a view into a larger image).  Writes n, keys, keysUn, descriptors, uRight, depth.
#include "ORBextractor.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> b;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    unsigned char tmp[65536];
    size_t r;
    while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) b.insert(b.end(), tmp, tmp + r);
    fclose(f);
    return b;
}

int main(int argc, char **argv)
{
    if (argc < 15) { fprintf(stderr, "usage: see the header of this file\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    const bool u16 = strcmp(argv[5], "u16") == 0, padded = atoi(argv[6]) != 0;
    const float scale = (float)atof(argv[7]), bf = (float)atof(argv[8]);
    const int nd = atoi(argv[13]);
    if (argc != 15 + nd) { fprintf(stderr, "bad argument count\n"); return 2; }
    std::vector<unsigned char> gray = slurp(argv[1]), draw = slurp(argv[2]);
    const size_t es = u16 ? 2 : 4, row = (size_t)w * es, step = padded ? row + 64 : row;
    if (gray.size() != (size_t)w * h || draw.size() != row * h) { fprintf(stderr, "input sizes\n"); return 2; }

    cv::Mat im(h, w, CV_8U);
    memcpy(im.data, &gray[0], gray.size());
    std::vector<unsigned char> dbuf(step * h + 64, 0xEE);   // padding bytes that must never be read as depth
    for (int y = 0; y < h; y++) memcpy(&dbuf[(size_t)y * step], &draw[(size_t)y * row], row);
    cv::Mat dep(1, 1, u16 ? CV_16U : CV_32F);
    dep.rows = h; dep.cols = w; dep.data = &dbuf[0]; dep.step = step;
    cv::Mat K(3, 3, CV_32F), D(nd, 1, CV_32F);
    memset(K.data, 0, 9 * 4);
    K.at<float>(0, 0) = (float)atof(argv[9]); K.at<float>(1, 1) = (float)atof(argv[10]);
    K.at<float>(0, 2) = (float)atof(argv[11]); K.at<float>(1, 2) = (float)atof(argv[12]); K.at<float>(2, 2) = 1.f;
    for (int i = 0; i < nd; i++) D.at<float>(i) = (float)atof(argv[14 + i]);

    ORB_SLAM2::ORBextractor ex(1000, 1.2f, 8, 20, 7);
    std::vector<cv::KeyPoint> keys, keysUn;
    cv::Mat desc;
    std::vector<float> ur, z;
    ex.ExtractRGBD(im, dep, scale, K, D, bf, keys, keysUn, desc, ur, z);
    const int n = (int)keys.size();
    if ((int)keysUn.size() != n || (int)ur.size() != n || (int)z.size() != n || (n && desc.rows != n)) { fprintf(stderr, "sizes\n"); return 3; }
    FILE *o = fopen(argv[14 + nd], "wb");
    if (!o) { perror("out"); return 2; }
    fwrite(&n, 4, 1, o);
    if (n) {
        fwrite(&keys[0], sizeof(cv::KeyPoint), n, o);
        fwrite(&keysUn[0], sizeof(cv::KeyPoint), n, o);
        for (int i = 0; i < n; i++) fwrite(desc.ptr<unsigned char>(i), 1, 32, o);
        fwrite(&ur[0], 4, n, o);
        fwrite(&z[0], 4, n, o);
    }
    fclose(o);
    return 0;
}
