// Driver of the reference's StereoImage::histogramNormalization for the golden fixture (tests/histnorm_ref.py links it
// with the reference's stereomapper/stereoimage.cpp, compiled unchanged over tests/histnorm/qt_stub/QObject).
//   ref_histnorm_harness <job>      job: int32 count, then per image int32 width, height, step and step * height bytes
// writes every image after the call, step * height bytes each, to stdout.
#include <stdio.h>

#include <vector>

#include "stereoimage.h"

void StereoImage::newStereoImageArrived() {}   // the signal's body (moc's job)

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    StereoImage si;
    for (int32_t i = 0; i < count; i++) {
        int32_t d[3];
        if (fread(d, 4, 3, f) != 3) return 2;
        std::vector<unsigned char> I((size_t)d[2] * (size_t)d[1]);
        if (fread(I.data(), 1, I.size(), f) != I.size()) return 2;
        si.histogramNormalization(I.data(), d[0], d[1], d[2]);
        if (fwrite(I.data(), 1, I.size(), stdout) != I.size()) return 2;
    }
    fclose(f);
    return 0;
}
