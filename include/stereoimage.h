/*
 * stereoimage.h -- Qt-free, source-compatible stand-in for stereomapper/stereoimage.h.
 *
 * class StereoImage with the reference's public section (:24-124): struct simage with its deep-copy semantics,
 * setImage (pairs a left and a right frame whose capture stamps differ by less than 10 ms), isRectified,
 * getStereoImage, pickedUp, timeDiff, and histogramNormalization(I, width, height, step) over the svh_histnorm_*
 * entries of svh_histnorm.h, so that the equalisation runs on the MI355X.
 *
 * Differences, all stated:
 *   - No Qt.  The signal newStereoImageArrived() is a callback: setNewStereoImageArrived(fn, user); setImage calls
 *     fn(user) where the reference emits.
 *   - The reference then blocks in `while (!_picked) usleep(1000);` until the receiving thread calls pickedUp().  That
 *     wait is NOT reproduced: setImage returns after the callback.  pickedUp() still sets the flag, and picked() reads
 *     it, so a caller that wants the hand-shake can wait on it on its own terms.
 *   - histogramNormalization keeps the reference's arithmetic bit for bit, including the byte wrap of its map (a flat
 *     1392x512 frame becomes 1 everywhere; see svh_histnorm.h).  It returns nothing, like the reference's; the status
 *     of the last call is lastStatus() (SVH_OK, SVH_ERR_NO_DEVICE, ...), and an image is untouched after a failure.
 *   - The struct `image` of a single camera initialises its step (the reference leaves it indeterminate).
 */
#ifndef STEREOIMAGE_H
#define STEREOIMAGE_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "svh_histnorm.h"

class StereoImage {
public:
    StereoImage()
        : _img_left(new image()), _img_right(new image()), _simg(new simage()), _picked(false), _arrived(0),
          _arrived_user(0), _hn(0), _hn_w(0), _hn_h(0), _status(SVH_OK) {}
    ~StereoImage() {
        delete _img_left;
        delete _img_right;
        delete _simg;
        svh_histnorm_destroy(_hn);
    }

    struct simage {
        unsigned char* I1;   // input images
        unsigned char* I2;
        float* D1;           // disparity maps
        float* D2;
        int width, height, step;
        timeval time;
        bool rectified;

        simage() : I1(0), I2(0), D1(0), D2(0), width(0), height(0), step(0), rectified(false) {
            time.tv_sec = 0;
            time.tv_usec = 0;
        }
        // a deep copy: step * height elements of every buffer the source holds
        simage(const simage& src)
            : I1(0), I2(0), D1(0), D2(0), width(src.width), height(src.height), step(src.step), time(src.time),
              rectified(src.rectified) {
            const size_t n = (size_t)src.step * (size_t)src.height;
            I1 = copy_of(src.I1, n);
            I2 = copy_of(src.I2, n);
            D1 = copy_of(src.D1, n);
            D2 = copy_of(src.D2, n);
        }
        ~simage() {
            free(I1);
            free(I2);
            free(D1);
            free(D2);
        }

    private:
        simage& operator=(const simage&);   // (the reference declares none; its implicit one would double free)
        template <class T>
        static T* copy_of(const T* p, size_t n) {
            if (!p) return 0;
            T* q = (T*)malloc(n * sizeof(T));
            memcpy(q, p, n * sizeof(T));
            return q;
        }
    };

    // one camera's frame (step * height bytes are copied); when the left and the right frame now held are less than
    // 10 ms apart and of one size, they become the stereo image and the callback runs
    void setImage(unsigned char* data, int width, int height, int step, bool cam_left, bool rectified,
                  timeval captured_time) {
        image* img = cam_left ? _img_left : _img_right;
        const size_t bytes = (size_t)step * (size_t)height;
        if (width != img->width || height != img->height || step != img->step) {
            free(img->data);
            img->data = (unsigned char*)malloc(bytes);
            img->width = width, img->height = height, img->step = step;
        }
        img->time = captured_time;
        memcpy(img->data, data, bytes);
        if (!(fabs(timeDiff(_img_left->time, _img_right->time)) < 10)) return;
        if (_img_left->width != _img_right->width || _img_left->height != _img_right->height ||
            _img_left->step != _img_right->step)
            return;
        if (_img_left->width != _simg->width || _img_left->height != _simg->height || _img_left->step != _simg->step) {
            free(_simg->I1);
            free(_simg->I2);
            _simg->I1 = (unsigned char*)malloc(bytes);
            _simg->I2 = (unsigned char*)malloc(bytes);
            _simg->width = _img_left->width, _simg->height = _img_left->height, _simg->step = _img_left->step;
        }
        _simg->time = _img_left->time;
        _simg->rectified = rectified;
        memcpy(_simg->I1, _img_left->data, bytes);
        memcpy(_simg->I2, _img_right->data, bytes);
        _picked = false;
        if (_arrived) _arrived(_arrived_user);
        // (the reference waits here for pickedUp(); see the head of this file)
    }
    bool isRectified() { return _simg->rectified; }
    simage* getStereoImage() { return _simg; }
    void pickedUp() { _picked = true; }

    // the reference's call: a host image of height rows of width bytes, step apart, equalised in place
    void histogramNormalization(unsigned char* I, const int& width, const int& height, const int& step) {
        (void)histogramNormalization(I, false, width, height, step);
    }

    // milliseconds from b to a
    float timeDiff(timeval a, timeval b) {
        return ((float)(a.tv_sec - b.tv_sec)) * 1e+3 + ((float)(a.tv_usec - b.tv_usec)) * 1e-3;
    }

    // ---- extension (not in the reference) ----
    void setNewStereoImageArrived(void (*fn)(void*), void* user) { _arrived = fn, _arrived_user = user; }
    bool picked() const { return _picked; }
    // the same call for an image in host or device memory; returns the status of svh_histnorm_apply
    int32_t histogramNormalization(unsigned char* I, bool on_device, int width, int height, int step) {
        if (!_hn || width != _hn_w || height != _hn_h) {
            svh_histnorm_destroy(_hn);
            _hn = svh_histnorm_create(width, height);
            _hn_w = width, _hn_h = height;
        }
        _status = _hn ? svh_histnorm_apply(_hn, I, on_device ? 1 : 0, step) : SVH_ERR_BAD_ARG;
        return _status;
    }
    int32_t lastStatus() const { return _status; }
    svh_histnorm* handle() { return _hn; }   // for the svh_histnorm_* taps and timing

private:
    StereoImage(const StereoImage&);
    StereoImage& operator=(const StereoImage&);

    struct image {
        unsigned char* data;
        int width, height, step;
        timeval time;
        image() : data(0), width(0), height(0), step(0) {
            time.tv_sec = 0;
            time.tv_usec = 0;
        }
        ~image() { free(data); }
    };

    image* _img_left;
    image* _img_right;
    simage* _simg;
    bool _picked;
    void (*_arrived)(void*);
    void* _arrived_user;
    svh_histnorm* _hn;
    int _hn_w, _hn_h;
    int32_t _status;
};

#endif   // STEREOIMAGE_H
