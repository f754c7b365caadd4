// Distorted COLMAP camera models of the ray generator (camera record modes 2 and 3, include/mipnerf_hip.h): a pixel's normalised
// DISTORTED image point (xd, yd) -> the camera-space direction of its ray, by inverting the model with a fixed number of Newton
// steps.  Plain templated C++ (T = float or double): kernels_ray.hip includes it for the device, a host program for the CPU
// (tests/camera_models_host.cpp), and both run the same operations in the same order.
//
//   mode 2, radial-tangential (COLMAP SIMPLE_RADIAL, RADIAL, OPENCV), k = (k1, k2, p1, p2):
//       r2 = x^2 + y^2,  radial = 1 + k1 r2 + k2 r2^2
//       distort(x, y) = (x radial + 2 p1 x y + p2 (r2 + 2 x^2),  y radial + 2 p2 x y + p1 (r2 + 2 y^2))
//     solve distort(xu, yu) = (xd, yd); direction (xu, -yu, -1) -- third component -1 like the pinhole modes.
//   mode 3, equidistant fisheye (COLMAP OPENCV_FISHEYE), k = (k1, k2, k3, k4):
//       thetad = |(xd, yd)|;  solve theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = thetad
//     direction (sin theta xd / thetad, -sin theta yd / thetad, -cos theta): of UNIT length, the only form that survives 90 degrees,
//     so t, near and far of such a camera are distances along the ray (multinerf's camera_utils does the same).
//
// CAMERA_NEWTON_STEPS steps, no data-dependent exit: the cost is uniform across a wavefront and the loop unrolls.  Started at the
// distorted point, 8 steps reach the float64 fixed point to 3e-16 and the float32 one to 2e-7 absolute on barrel and pincushion sets
// up to k1 = -0.3 at a normalised radius of 0.98 (6 steps already do).  A step whose Jacobian determinant (derivative, for the fisheye) is
// below 1e-9 in magnitude is a zero step; a non-finite result is replaced by the distorted point, so no NaN leaves this header.
// With all-zero coefficients every step is exactly zero and mode 2 returns (xd, yd) bit for bit: the mode-1 direction.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CAMERA_MODELS_FN __host__ __device__ __forceinline__
#else
#define CAMERA_MODELS_FN inline
#endif

namespace camera_models {

constexpr int CAMERA_NEWTON_STEPS = 8;
constexpr int NUM_CAMERA_MODES = 4;          // 0 Blender focal, 1 pix2cam, 2 radial-tangential, 3 equidistant fisheye

// COLMAP's radial-tangential forward model (also the tests' way back from a direction to a pixel)
template <typename T>
CAMERA_MODELS_FN void distort_radial(const T* k, T x, T y, T& xo, T& yo) {
    const T r2 = x * x + y * y;
    const T radial = T(1) + k[0] * r2 + k[1] * r2 * r2;
    xo = x * radial + T(2) * k[2] * x * y + k[3] * (r2 + T(2) * x * x);
    yo = y * radial + T(2) * k[3] * x * y + k[2] * (r2 + T(2) * y * y);
}

template <typename T>
CAMERA_MODELS_FN void undistort_radial(const T* k, T xd, T yd, T& xu, T& yu) {
    using std::isfinite;
    T x = xd, y = yd;
#pragma unroll
    for (int it = 0; it < CAMERA_NEWTON_STEPS; ++it) {
        T fx, fy;
        distort_radial<T>(k, x, y, fx, fy);
        fx -= xd;
        fy -= yd;
        const T r2 = x * x + y * y;
        const T radial = T(1) + k[0] * r2 + k[1] * r2 * r2;
        const T dradial = T(2) * (k[0] + T(2) * k[1] * r2);            // d radial / d x = dradial * x
        const T j00 = radial + dradial * x * x + T(2) * k[2] * y + T(6) * k[3] * x;
        const T j01 = dradial * x * y + T(2) * k[2] * x + T(2) * k[3] * y;          // = j10
        const T j11 = radial + dradial * y * y + T(2) * k[3] * x + T(6) * k[2] * y;
        const T det = j00 * j11 - j01 * j01;
        const bool ok = det > T(1e-9) || det < T(-1e-9);
        const T inv = T(1) / (ok ? det : T(1));
        const T sx = ok ? (j11 * fx - j01 * fy) * inv : T(0);
        const T sy = ok ? (j00 * fy - j01 * fx) * inv : T(0);
        x -= sx;
        y -= sy;
    }
    const bool fin = isfinite(x) && isfinite(y);
    xu = fin ? x : xd;
    yu = fin ? y : yd;
}

// theta_d(theta) of the equidistant fisheye model
template <typename T>
CAMERA_MODELS_FN T distort_fisheye_theta(const T* k, T th) {
    const T t2 = th * th;
    return th * (T(1) + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}

template <typename T>
CAMERA_MODELS_FN T undistort_fisheye_theta(const T* k, T thd) {
    using std::isfinite;
    T th = thd;
#pragma unroll
    for (int it = 0; it < CAMERA_NEWTON_STEPS; ++it) {
        const T t2 = th * th;
        const T f = distort_fisheye_theta<T>(k, th) - thd;
        const T df = T(1) + t2 * (T(3) * k[0] + t2 * (T(5) * k[1] + t2 * (T(7) * k[2] + t2 * (T(9) * k[3]))));
        const bool ok = df > T(1e-9) || df < T(-1e-9);
        th -= ok ? f / df : T(0);
    }
    return isfinite(th) ? th : thd;
}

// mode 2 or 3: the normalised distorted point (xd, yd) (y down, as COLMAP) -> camera direction c (x right, y up, looking down -z)
template <typename T>
CAMERA_MODELS_FN void undistorted_direction(int mode, const T* k, T xd, T yd, T c[3]) {
    using std::cos;
    using std::sin;
    using std::sqrt;
    if (mode == 2) {
        T xu, yu;
        undistort_radial<T>(k, xd, yd, xu, yu);
        c[0] = xu;
        c[1] = -yu;
        c[2] = T(-1);
    } else {
        const T thd = sqrt(xd * xd + yd * yd);
        const T th = undistort_fisheye_theta<T>(k, thd);
        const T s = thd < T(1e-8) ? T(1) : sin(th) / thd;
        c[0] = s * xd;
        c[1] = -(s * yd);
        c[2] = -cos(th);
    }
}

}  // namespace camera_models
