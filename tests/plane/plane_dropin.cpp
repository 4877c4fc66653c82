// The plane step of StereoThread::run (stereomapper/stereothread.cpp:155-163) written against the reference's
// planeestimation.h, compiled with include/ alone on the include path:
//     _plane->computeTransformationFromDisparityMap(D1, width, height, width, f, cu, cv, base);
//     _H_init = Matrix::inv(_plane->getTransformation());
//     _H_total = _H_init * _H_total;
//
//   plane_dropin <map> width height f cu cv base seed
// <map>: width * height floats.  Runs the reference's call (seeded by the clock) and the seeded extension, and writes
// for the seeded call: _plane_d (3), _plane_e (3), _H (16), inv(_H) * I (16) as text with 17 digits, then the pitch.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "planeestimation.h"

int main(int argc, char** argv) {
    if (argc < 9) {
        fprintf(stderr, "usage: plane_dropin MAP width height f cu cv base seed\n");
        return 1;
    }
    const int32_t width = atoi(argv[2]), height = atoi(argv[3]);
    const float f = (float)atof(argv[4]), cu = (float)atof(argv[5]), cv = (float)atof(argv[6]), base = (float)atof(argv[7]);
    std::vector<float> D((size_t)width * height);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp || fread(D.data(), 4, D.size(), fp) != D.size()) return 2;
    fclose(fp);

    PlaneEstimation* _plane = new PlaneEstimation();
    Matrix _H_total = Matrix::eye(4);
    // the reference's call
    _plane->computeTransformationFromDisparityMap(D.data(), width, height, width, f, cu, cv, base);
    Matrix _H_init = Matrix::inv(_plane->getTransformation());
    // the seeded extension
    const int32_t rc = _plane->computeTransformationFromDisparityMap(D.data(), false, width, height, width, f, cu, cv,
                                                                     base, (uint32_t)strtoul(argv[8], 0, 10));
    if (rc < 0) return 3;
    _H_init = Matrix::inv(_plane->getTransformation());
    _H_total = _H_init * _H_total;
    Matrix pd = _plane->getPlaneDsi(), pe = _plane->getPlaneEuclidean(), H = _plane->getTransformation();
    for (int i = 0; i < 3; i++) printf("%.17g ", pd._val[i][0]);
    printf("\n");
    for (int i = 0; i < 3; i++) printf("%.17g ", pe._val[i][0]);
    printf("\n");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) printf("%.17g ", H._val[i][j]);
    printf("\n");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) printf("%.17g ", _H_total._val[i][j]);
    printf("\n%.9g\n", (double)_plane->getPitch());
    delete _plane;
    return 0;
}
