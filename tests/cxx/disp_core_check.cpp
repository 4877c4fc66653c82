// CPU check of the 16-bit disparity encoding (stereo-vision_amd/csrc/disp_core.h compiled by g++ alone): reads n
// float32 values from the file given, writes n uint16 (u16 of each) and then n float32 (f32 of each of those) to stdout.
// tests/test_disp_u16.py builds it on the spot and compares with the numpy restatement tests/disp_u16_ref.py.
#include <stdio.h>

#include <vector>

#include "../../stereo-vision_amd/csrc/disp_core.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> d;
    float buf[4096];
    for (size_t got; (got = fread(buf, sizeof(float), 4096, f)) > 0;) d.insert(d.end(), buf, buf + got);
    fclose(f);
    std::vector<uint16_t> v(d.size());
    std::vector<float> back(d.size());
    for (size_t i = 0; i < d.size(); i++) {
        v[i] = svh::disp::u16(d[i]);
        back[i] = svh::disp::f32(v[i]);
    }
    if (fwrite(v.data(), sizeof(uint16_t), v.size(), stdout) != v.size()) return 1;
    if (fwrite(back.data(), sizeof(float), back.size(), stdout) != back.size()) return 1;
    return 0;
}
