/*
 * view2d.h -- Qt-free drop-in for stereomapper's View2D (stereomapper/view2d.h, view2d.cpp) over the C-ABI of
 * svh_view2d.h: the public names of the reference's widget, the pane rendered on the device.
 *
 * Differences from the widget, all stated in svh_view2d.h: no window (grabFrameBuffer() returns the image a paint
 * would show, width * height * 3 bytes, row 0 = top), no multisampling, and a binary-PPM writer instead of Qt's image
 * files.  setDisparity is an addition: the colour map of StereoThread and setColorImage in one pass, from a host or a
 * device pointer.  Equality of the images with any OpenGL implementation is not verified.
 */
#ifndef VIEW2D_H
#define VIEW2D_H

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "matcher.h"
#include "svh_view2d.h"

class View2D {
public:
    // the reference's widget is sized by its layout; resizeGL changes it
    explicit View2D(int32_t width = 320, int32_t height = 240) : _width(width), _height(height) {
        _view = svh_view2d_create(width, height);
    }
    ~View2D() { svh_view2d_destroy(_view); }
    View2D(const View2D&) = delete;
    View2D& operator=(const View2D&) = delete;

    bool valid() const { return _view != 0; }   // false: no HIP device (svh_last_error())

    void setImage(unsigned char* data, int width, int height) {
        const int32_t dims[3] = {width, height, width};
        svh_view2d_set_image(_view, data, dims, 0);
    }
    void setColorImage(float* data, int width, int height) { svh_view2d_set_color_image(_view, data, width, height, 0); }
    void setMatches(const std::vector<Matcher::p_match>& m, const std::vector<bool>& i, bool l) {
        if (i.size() != m.size()) return;
        std::vector<uint8_t> flags(i.size());
        for (size_t k = 0; k < i.size(); k++) flags[k] = i[k] ? 1 : 0;
        svh_view2d_set_matches(_view, m.empty() ? 0 : reinterpret_cast<const svh_p_match*>(&m[0]), (int32_t)m.size(),
                               flags.empty() ? 0 : &flags[0], l ? 1 : 0, 0);
    }
    void clearMatches() { svh_view2d_clear_matches(_view); }
    void resizeGL(int width, int height) {
        if (svh_view2d_resize(_view, width, height) == 0) _width = width, _height = height;
    }

    // frames and maps where the chain left them in device memory
    void setImageDevice(const uint8_t* data, int width, int height, int pitch) {
        const int32_t dims[3] = {width, height, pitch};
        svh_view2d_set_image(_view, data, dims, 1);
    }
    void setDisparity(const float* D, int width, int height, bool on_device = false) {
        svh_view2d_set_disparity(_view, D, width, height, on_device ? 1 : 0);
    }

    int32_t width() const { return _width; }
    int32_t height() const { return _height; }

    // paintGL + grabFrameBuffer; returns SVH_OK or a negative SVH_ERR_*
    int32_t render(uint8_t* rgb) { return svh_view2d_render(_view, rgb, 0); }
    std::vector<uint8_t> grabFrameBuffer() {
        std::vector<uint8_t> rgb((size_t)_width * (size_t)_height * 3);
        if (render(rgb.data()) != 0) rgb.clear();
        return rgb;
    }
    // the pane as a binary PPM (P6)
    bool writePPM(const std::string& path) {
        const std::vector<uint8_t> rgb = grabFrameBuffer();
        if (rgb.empty()) return false;
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) return false;
        fprintf(f, "P6\n%d %d\n255\n", (int)_width, (int)_height);
        const bool ok = fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
        return fclose(f) == 0 && ok;
    }

private:
    svh_view2d* _view;
    int32_t _width, _height;
};

#endif
