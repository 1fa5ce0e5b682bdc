// The pinhole camera that the rasteriser (mesh_raster.hip) and the TSDF fusion (mesh_tsdf.hip) share, in one definition, so that a lattice
// point lands in the pixel whose rasterised or rendered depth it is compared with: the cameras of cnerf_generate_rays, the arithmetic of
// include/customnerf_hip.h (the rasteriser's block): float32, one rounding per written operation, in the order written.
#pragma once
#include "mesh_common.h"

namespace {

struct MeshCam {
    float m[3][4];                                               // c2w, row-major; t = column 3
    float fx, fy, cx, cy, near;
    int convention;                                              // 0 'nerfstudio' (looks down -z, y up), 1 'ngp' (+z forward, y down)
};

inline MeshCam mesh_cam(const float *c2w_host, float fx, float fy, float cx, float cy, float near, int convention) {
    MeshCam cam;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) cam.m[r][k] = c2w_host[4 * r + k];
    cam.fx = fx;
    cam.fy = fy;
    cam.cx = cx;
    cam.cy = cy;
    cam.near = near;
    cam.convention = convention;
    return cam;
}

// what every entry point that takes this camera refuses (CNERF_EINVAL)
inline bool mesh_cam_ok(float fx, float fy, float cx, float cy, float near, int convention) {
    return fabsf(fx) < INFINITY && fabsf(fy) < INFINITY && fx != 0.0f && fy != 0.0f && fabsf(cx) < INFINITY && fabsf(cy) < INFINITY &&
           fabsf(near) < INFINITY && convention >= 0 && convention <= 1;
}

// d = p - t -> camera-axis depth z and the pixel coordinates (X, Y); the caller decides what z < near and non-finite values mean
__device__ __forceinline__ void mesh_cam_project(const MeshCam &cam, float d0, float d1, float d2, float &z, float &X, float &Y) {
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (cam.m[0][k] * d0 + cam.m[1][k] * d1) + cam.m[2][k] * d2;
    z = cam.convention == 0 ? -c[2] : c[2];
    const float sy = cam.convention == 0 ? -1.0f : 1.0f;
    X = cam.cx + cam.fx * (c[0] / z);
    Y = cam.cy + sy * (cam.fy * (c[1] / z));
}

}  // namespace
