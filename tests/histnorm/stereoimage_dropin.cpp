// A caller written against the reference's StereoImage, compiled against include/stereoimage.h alone and linked with
// libsvhip.so (tests/test_histnorm.py builds it into a temporary directory).
//   stereoimage_dropin [gpu]     with `gpu` the equalisation must succeed; without a device it must refuse and leave
//                                the image untouched.  Prints one line per check; exit status 0 when all hold.
#include <stdio.h>

#include <vector>

#include "stereoimage.h"

static int g_failed = 0;
#define CHECK(what)                                   \
    do {                                              \
        const bool ok_ = (what);                      \
        printf("%s  %s\n", ok_ ? "ok  " : "FAIL", #what); \
        if (!ok_) g_failed++;                         \
    } while (0)

static void arrived(void* user) { ++*(int*)user; }

static timeval stamp(long sec, long usec) {
    timeval t;
    t.tv_sec = sec;
    t.tv_usec = usec;
    return t;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && argv[1][0] == 'g';
    StereoImage si;
    int calls = 0;
    si.setNewStereoImageArrived(arrived, &calls);

    CHECK(si.timeDiff(stamp(12, 500000), stamp(10, 250000)) == 2250.0f);
    CHECK(si.getStereoImage()->I1 == 0 && si.getStereoImage()->width == 0);

    const int w = 5, h = 3, step = 8;
    std::vector<unsigned char> L(step * h), R(step * h);
    for (int i = 0; i < step * h; i++) L[i] = (unsigned char)i, R[i] = (unsigned char)(100 + i);
    si.setImage(L.data(), w, h, step, true, true, stamp(100, 0));
    CHECK(calls == 0);                                               // no right frame yet
    si.setImage(R.data(), w, h, step, false, true, stamp(100, 20000));
    CHECK(calls == 0);                                               // 20 ms apart
    si.setImage(R.data(), w, h, step, false, true, stamp(100, 9000));
    CHECK(calls == 1 && !si.picked() && si.isRectified());           // 9 ms apart: a stereo frame, and no wait
    si.pickedUp();
    CHECK(si.picked());
    StereoImage::simage* s = si.getStereoImage();
    CHECK(s->width == w && s->height == h && s->step == step && s->time.tv_sec == 100 && s->time.tv_usec == 0);
    CHECK(memcmp(s->I1, L.data(), L.size()) == 0 && memcmp(s->I2, R.data(), R.size()) == 0 && s->D1 == 0);
    {
        StereoImage::simage c(*s);                                   // a deep copy
        CHECK(c.I1 != s->I1 && c.I2 != s->I2 && memcmp(c.I1, s->I1, L.size()) == 0 && memcmp(c.I2, s->I2, R.size()) == 0);
        CHECK(c.width == w && c.step == step && c.rectified && c.D2 == 0);
        c.I1[0] = 77;
        CHECK(s->I1[0] == L[0]);
    }
    si.setImage(L.data(), w, h, step, true, false, stamp(100, 1000));
    CHECK(calls == 2 && !si.picked() && !si.isRectified());
    si.setImage(L.data(), w + 1, h, step, true, false, stamp(100, 2000));
    CHECK(calls == 2);                                               // the two cameras differ in size

    // the reference's call on a flat 1392x512 frame with rows 3 bytes longer: every pixel becomes 1 (the byte wrap)
    const int W = 1392, H = 512, S = W + 3;
    std::vector<unsigned char> I((size_t)S * H, 0x5A);
    for (int v = 0; v < H; v++) memset(&I[(size_t)v * S], 100, W);
    si.histogramNormalization(I.data(), W, H, S);
    const int32_t rc = si.lastStatus();
    printf("histogramNormalization: status %d (%s)\n", rc, rc ? svh_last_error() : "ok");
    bool pixels_1 = true, pixels_100 = true, padding = true;
    for (int v = 0; v < H; v++)
        for (int u = 0; u < S; u++) {
            const unsigned char b = I[(size_t)v * S + u];
            if (u >= W) padding = padding && b == 0x5A;
            else pixels_1 = pixels_1 && b == 1, pixels_100 = pixels_100 && b == 100;
        }
    CHECK(padding);
    if (gpu) CHECK(rc == SVH_OK && pixels_1);
    else CHECK((rc == SVH_OK && pixels_1) || (rc == SVH_ERR_NO_DEVICE && pixels_100));
    CHECK(si.histogramNormalization(I.data(), false, 0, H, S) == SVH_ERR_BAD_ARG);
    printf("%s\n", g_failed ? "FAILED" : "all ok");
    return g_failed ? 1 : 0;
}
