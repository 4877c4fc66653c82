/*
 * view3d.h -- Qt-free drop-in for stereomapper's View3D (stereomapper/view3d.h, view3d.cpp) over the C-ABI of
 * svh_view.h: the public names of the reference's widget, the map accumulated and rendered on the device.
 *
 * Differences from the widget, all stated in svh_view.h: no window (render() returns the image a paint would show),
 * no mouse, no multisampling, no background wall (its two setters are kept and do nothing), and recordings are binary
 * PPM files in a directory the caller names instead of PNG files in the author's home directory.  Equality of the
 * images with any OpenGL implementation is not verified.
 */
#ifndef VIEW3D_H
#define VIEW3D_H

#include <stdint.h>
#include <stdio.h>

#include <iostream>
#include <string>
#include <vector>

#include "matrix.h"
#include "svh_view.h"

class View3D {
public:
    struct point_3d {
        float x, y, z;
        float val;
        point_3d(float x, float y, float z, float val) : x(x), y(y), z(z), val(val) {}
    };

    // the reference's widget is sized by its layout: 320 x 480 in the recordings
    explicit View3D(int32_t width = 320, int32_t height = 480) : _width(width), _height(height) {
        _view = svh_view_create(width, height);
        svh_view_pose_default(&_pose_curr);
        _flags.show_cams = 1, _flags.show_grid = 1, _flags.white = 0;
    }
    ~View3D() { svh_view_destroy(_view); }
    View3D(const View3D&) = delete;
    View3D& operator=(const View3D&) = delete;

    bool valid() const { return _view != 0; }   // false: no HIP device (svh_last_error())

    void addCamera(Matrix H_total, float s, bool keyframe) {
        double H[16];
        if (H_total._m != 4 || H_total._n != 4) return;
        H_total.getData(H);
        svh_view_add_camera(_view, H, s, keyframe ? 1 : 0);
    }

    void addPoints(std::vector<std::vector<point_3d>> p) {
        std::vector<const float*> ptr(p.size());
        std::vector<int64_t> n(p.size());
        for (size_t i = 0; i < p.size(); i++) {
            ptr[i] = p[i].empty() ? 0 : &p[i][0].x;   // point_3d is four packed floats
            n[i] = (int64_t)p[i].size();
        }
        svh_view_add_points(_view, ptr.data(), n.data(), (int32_t)p.size(), 0);
    }

    // the lists of the frame svh_map_add has just processed, without leaving the device
    void addPoints(svh_map* map) { svh_view_add_map(_view, map); }

    // additions to the widget's interface (svh_view.h): keep the first-drawn point of every cube of side `voxel`;
    // returns the number of points left or a negative SVH_ERR_*
    int64_t thin(float voxel) {
        svh_view_thin_stats st;
        const int32_t rc = svh_view_thin(_view, voxel, &st);
        return rc < 0 ? (int64_t)rc : st.after;
    }
    // ... and the map itself: the lists as they are held, empty ones included
    std::vector<std::vector<point_3d>> getPoints() {
        std::vector<std::vector<point_3d>> p((size_t)svh_view_count(_view, 0));
        for (size_t i = 0; i < p.size(); i++) {
            const int64_t n = svh_view_list_len(_view, (int32_t)i);
            if (n <= 0) continue;
            p[i].resize((size_t)n, point_3d(0, 0, 0, 0));
            svh_view_get_points(_view, (int32_t)i, &p[i][0].x, n, 0);
        }
        return p;
    }

    void clearAll() { svh_view_clear(_view); }
    void setBackgroundWallFlag(bool) {}        // out of scope, see svh_view.h
    void setBackgroundWallPosition(float) {}
    void setShowCamerasFlag(bool show_cam_flag_) { _flags.show_cams = show_cam_flag_; svh_view_set_flags(_view, &_flags); }
    void setGridFlag(bool show_grid_flag_) { _flags.show_grid = show_grid_flag_; svh_view_set_flags(_view, &_flags); }
    void setWhiteFlag(bool show_white_flag_) { _flags.white = show_white_flag_; svh_view_set_flags(_view, &_flags); }
    void addPose() { _poses.push_back(_pose_curr); std::cout << "Poses: " << _poses.size() << std::endl; }
    void delPose() { if (_poses.size() > 0) _poses.pop_back(); std::cout << "Poses: " << _poses.size() << std::endl; }

    // what the mouse does in the widget
    void setPose(const svh_view_pose& pose) { _pose_curr = pose; svh_view_set_pose(_view, &_pose_curr); }
    const svh_view_pose& getPose() const { return _pose_curr; }
    void resize(int32_t width, int32_t height) {
        if (svh_view_resize(_view, width, height) == 0) _width = width, _height = height;
    }
    int32_t width() const { return _width; }
    int32_t height() const { return _height; }

    // paintGL + grabFrameBuffer: width * height * 3 bytes, row 0 = top; returns SVH_OK or a negative SVH_ERR_*
    int32_t render(uint8_t* rgb) {
        svh_view_set_pose(_view, &_pose_curr);
        return svh_view_render(_view, rgb, 0);
    }

    // playPoses(record): with a directory, every frame is written there as img_<width>_<height>_%06d.ppm.
    // Returns the number of frames or a negative SVH_ERR_*.
    int64_t playPoses(const std::string& record_dir = std::string()) {
        const int64_t frames = _poses.size() < 2 ? 0 : 51 * (int64_t)(_poses.size() - 1);
        const size_t bytes = (size_t)_width * (size_t)_height * 3;
        std::vector<uint8_t> rgb(record_dir.empty() ? 0 : bytes * (size_t)frames);
        const int64_t n = svh_view_play_poses(_view, _poses.data(), (int32_t)_poses.size(), rgb.empty() ? 0 : rgb.data(),
                                              record_dir.empty() ? 0 : frames, 0);
        if (n <= 0) return n;
        std::vector<svh_view_pose> seq((size_t)n);
        svh_view_play_sequence(_poses.data(), (int32_t)_poses.size(), seq.data(), n);
        _pose_curr = seq.back();
        for (int64_t k = 0; !record_dir.empty() && k < n; k++) {
            char name[64];
            snprintf(name, sizeof(name), "/img_%d_%d_%06d.ppm", (int)_width, (int)_height, (int)k);
            const std::string path = record_dir + name;
            std::cout << "Storing " << path << std::endl;
            FILE* f = fopen(path.c_str(), "wb");
            if (!f) return -1;
            fprintf(f, "P6\n%d %d\n255\n", (int)_width, (int)_height);
            fwrite(rgb.data() + (size_t)k * bytes, 1, bytes, f);
            fclose(f);
        }
        return n;
    }

    // recordHuman: the fly-through -45 .. +45 .. -45 degrees around the current pose, recorded into record_dir
    int64_t recordHuman(const std::string& record_dir) {
        _poses.clear();
        svh_view_pose pose1 = _pose_curr, pose2 = _pose_curr;
        pose1.roty -= 45;
        pose2.roty += 45;
        _poses.push_back(pose1);
        _poses.push_back(pose2);
        _poses.push_back(pose1);
        return playPoses(record_dir);
    }

private:
    svh_view* _view;
    int32_t _width, _height;
    std::vector<svh_view_pose> _poses;
    svh_view_pose _pose_curr;
    svh_view_flags _flags;
};

#endif
