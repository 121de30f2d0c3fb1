// orbx_trig.h -- the keypoint angle and its sine / cosine as k_orient_describe evaluates them (orbx_kernels.hip), in a header of their own so that
// tests/test_orient_trig_host.py can compile the same bodies for the CPU and compare them bit for bit with oracle/prims.h.  No HIP and none of the
// library's other headers; every translation unit that includes it is built with -ffp-contract=off (no product and sum may fuse).
//
// Both functions are BRANCH-FREE: the kernel runs them on one lane per keypoint of a workgroup, and keypoints that took different sides of a branch
// made the wave run both sides (two float divisions, two polynomial pairs in double).  Every lane now executes the one sequence below, which holds the
// same float / double operations on the same operands as the branching forms of oracle/prims.h (op_fast_atan2, op_sincosf); the choices are selects.
#ifndef ORBX_TRIG_H
#define ORBX_TRIG_H

#include <stdint.h>

#ifdef __HIPCC__
#define ORBX_TRIG_FN __device__ __forceinline__
#else
#define ORBX_TRIG_FN static inline
#endif

// cv::fastAtan2 (degrees, [0, 360]) of IC_Angle's moments: numerator and denominator are selected, then ONE division and ONE polynomial; `90 - a`
// is a select as well.
ORBX_TRIG_FN float fast_atan2_deg(float y, float x)
{
    const float scale = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
                p7 = -0.04432655554792128f * scale;
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const bool steep = !(ax >= ay);
    const float c = (steep ? ax : ay) / ((steep ? ay : ax) + 2.220446049250313e-16f);
    const float c2 = c * c;
    float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    a = steep ? 90.f - a : a;
    a = x < 0 ? 180.f - a : a;
    a = y < 0 ? 360.f - a : a;
    return a;
}

// The two polynomial forms of glibc 2.35's sinf / cosf (sysdeps/ieee754/flt-32/s_sincosf.h, __sincosf_table[0]; table[1] negates the cosine
// coefficients: neg), in double, rounded to float once.
ORBX_TRIG_FN float sinf_poly_d(double x, double x2)
{
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    const double x3 = x * x2, t1 = s2 + x2 * s3, x7 = x3 * x2, s = x + x3 * s1;
    return (float)(s + x7 * t1);
}
ORBX_TRIG_FN float cosf_poly_d(double x2, bool neg)
{
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10, c4 = 0x1.99343027bf8c3p-16;
    const double k0 = neg ? -c0 : c0, k1 = neg ? -c1 : c1, k2 = neg ? -c2 : c2, k3 = neg ? -c3 : c3, k4 = neg ? -c4 : c4;
    const double x4 = x2 * x2, u2 = k3 + x2 * k4, u1 = k0 + x2 * k1, x6 = x4 * x2, c = u1 + x4 * k2;
    return (float)(c + x6 * u2);
}

// sin / cos of the keypoint angle as the libm that the reference calls rounds them (oracle/prims.h op_sincosf, tests/test_sincos.py), for
// |y| < 120.  glibc branches three ways; here
//   |y| < pi/4 (glibc's own polynomial call without a reduction) is the general path with n = 0: y * (2/pi) 2^24 < 2^23, so the rounded quotient
//       is 0, and x - 0 * (pi/2) and x * 1.0 are exact;
//   every call needs exactly one sine form and one cosine form of the same reduced argument - n odd swaps which of them is the sine;
//   |y| < 2^-12 keeps its own result (y, 1) as the last select.
ORBX_TRIG_FN void sincosf_glibc(float y, float &sn, float &cs)
{
    uint32_t yb;
    __builtin_memcpy(&yb, &y, 4);
    const uint32_t top = (yb >> 20) & 0x7ff;      // abstop12
    double x = y;
    const double r = x * 0x1.45F306DC9C883p+23;
    const int n = ((int)r + 0x800000) >> 24;
    x = x - n * 0x1.921FB54442D18p0;
    const double sgn = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;
    const double xs = x * sgn, x2 = x * x;
    const float s = sinf_poly_d(xs, x2), c = cosf_poly_d(x2, (n & 2) != 0);
    const bool odd = (n & 1) != 0, tiny = top < ((0x39800000u >> 20) & 0x7ff);      // |y| < 2^-12
    sn = tiny ? y : odd ? c : s;
    cs = tiny ? 1.0f : odd ? s : c;
}

#endif
