// The overlay on NV12 frames, host side, once, for fid_draw_faces_nv12_host (draw.hip) and the stand-alone sanitizer driver
// (tests/draw_nv12_host_driver.cpp): one face's pixel set (draw_core.h) painted onto the two planes of one frame with the forward colour
// definition (yuv_core.h).  The definition is include/faceid.h's (fid_draw_faces_nv12).  Plain inline functions, no HIP runtime call;
// compiles with a host-only compiler.
#pragma once
#include "draw_core.h"
#include "yuv_core.h"

// One face onto the frame whose Y plane starts at yp and whose UV plane starts at uvp, rows `pitch` bytes apart: every covered pixel sets its
// Y byte and the (U, V) pair of its 2 x 2 group.  Faces painted in ascending order leave each Y byte with its last covering face and each
// pair with the last face that covers any pixel of its group.  Writes yp[y * pitch + x] and uvp[(y >> 1) * pitch + (x & ~1) + {0, 1}] of
// covered pixels (x, y), which the clipped extent keeps inside the frame; returns how many pixels it covered.
inline long fid_draw_face_nv12_host(const fid_draw_face *fc, const fid_yuv_fwd &k, uint8_t *yp, uint8_t *uvp, int pitch, int r, int t,
                                    const uint8_t *font) {
    int yuv[3];
    fid_yuv_of_colour(k, fc->bgr[0], fc->bgr[1], fc->bgr[2], yuv);
    long lit = 0;
    for (int y = fc->ey0; y <= fc->ey1; y++)
        for (int x = fc->ex0; x <= fc->ex1; x++)
            if (fid_draw_covers(fc, x, y, r, t, font)) {
                yp[(size_t)y * (size_t)pitch + (size_t)x] = (uint8_t)yuv[0];
                uint8_t *c = uvp + (size_t)(y >> 1) * (size_t)pitch + (size_t)(x & ~1);
                c[0] = (uint8_t)yuv[1]; c[1] = (uint8_t)yuv[2];
                lit++;
            }
    return lit;
}
