// orbx_sim3_group.h -- g2o/types/sim3.h and the Eigen quaternion routines it uses, operation by operation, as device functions: shared by
// orbx_optimize_sim3.hip (Optimizer::OptimizeSim3) and orbx_essential_graph.hip (Optimizer::OptimizeEssentialGraph).  Every product, sum and
// quotient is its own IEEE operation (-ffp-contract=off); tests/optsim3_ref.py restates them in the same order.
#ifndef ORBX_SIM3_GROUP_H
#define ORBX_SIM3_GROUP_H

#include <hip/hip_runtime.h>
#include <math.h>

struct OsSim3 { double q[4]; double t[3]; double s; };      // q = (x, y, z, w) like Eigen's coeffs()

// ---- sim3.h / Eigen, operation by operation -------------------------------------------------------------------------------------------
__device__ __forceinline__ void os_quat_from_R(const double (&R)[9], double (&q)[4])      // Eigen::Quaterniond(Matrix3d)
{
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else if (!(R[4] > R[0]) && !(R[8] > R[0])) {      // i = 0, j = 1, k = 2
        t = sqrt(((R[0] - R[4]) - R[8]) + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[7] - R[5]) * t; q[1] = (R[3] + R[1]) * t; q[2] = (R[6] + R[2]) * t;
    } else if (R[4] > R[0] && !(R[8] > R[4])) {          // i = 1, j = 2, k = 0
        t = sqrt(((R[4] - R[8]) - R[0]) + 1.0);
        q[1] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[2] - R[6]) * t; q[2] = (R[7] + R[5]) * t; q[0] = (R[1] + R[3]) * t;
    } else {                                               // i = 2, j = 0, k = 1
        t = sqrt(((R[8] - R[0]) - R[4]) + 1.0);
        q[2] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[3] - R[1]) * t; q[0] = (R[2] + R[6]) * t; q[1] = (R[5] + R[7]) * t;
    }
}

__device__ __forceinline__ void os_quat_to_R(const double (&q)[4], double (&R)[9])      // Quaterniond::toRotationMatrix
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

__device__ __forceinline__ void os_rotate(const double (&q)[4], const double (&v)[3], double (&o)[3])      // Quaterniond * Vector3d
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    o[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
    o[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
    o[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}

__device__ __forceinline__ void os_map(const OsSim3 &S, const double (&v)[3], double (&o)[3])      // s * (r * xyz) + t
{
    double r[3];
    os_rotate(S.q, v, r);
    o[0] = S.s * r[0] + S.t[0]; o[1] = S.s * r[1] + S.t[1]; o[2] = S.s * r[2] + S.t[2];
}

__device__ __forceinline__ void os_mul(const OsSim3 &a, const OsSim3 &b, OsSim3 &o)      // Sim3::operator*: the quaternion is never renormalised
{
    const double *p = a.q, *r = b.q;
    o.q[3] = ((p[3] * r[3] - p[0] * r[0]) - p[1] * r[1]) - p[2] * r[2];
    o.q[0] = ((p[3] * r[0] + p[0] * r[3]) + p[1] * r[2]) - p[2] * r[1];
    o.q[1] = ((p[3] * r[1] + p[1] * r[3]) + p[2] * r[0]) - p[0] * r[2];
    o.q[2] = ((p[3] * r[2] + p[2] * r[3]) + p[0] * r[1]) - p[1] * r[0];
    double rt[3];
    os_rotate(a.q, b.t, rt);
    o.t[0] = a.s * rt[0] + a.t[0]; o.t[1] = a.s * rt[1] + a.t[1]; o.t[2] = a.s * rt[2] + a.t[2];
    o.s = a.s * b.s;
}

__device__ __forceinline__ void os_inverse(const OsSim3 &a, OsSim3 &o)      // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
{
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double f = -1.0 / a.s;
    const double v[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    os_rotate(o.q, v, o.t);
    o.s = 1.0 / a.s;
}

// the elementary functions os_exp calls: the device library's by default; a caller that pins them passes its own (orbx_essential_graph.hip)
struct OsLibm {
    static __device__ __forceinline__ double exp_(double x) { return exp(x); }
    static __device__ __forceinline__ double sin_(double x) { return sin(x); }
    static __device__ __forceinline__ double cos_(double x) { return cos(x); }
};

template <class M = OsLibm>
__device__ __forceinline__ void os_exp(const double (&u)[7], OsSim3 &o)      // Sim3(const Vector7d &), sim3.h:70-142
{
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double Om[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double Om2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    o.s = M::exp_(sigma);
    const double eps = 0.00001;
    double A, B, C, R[9];
    const bool smallT = theta < eps;
    double ca = 1.0, cb = 1.0;      // R = I + ca Omega + cb Omega2
    if (!smallT) { ca = M::sin_(theta) / theta; cb = (1.0 - M::cos_(theta)) / (theta * theta); }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        R[k] = smallT ? (I + Om[k]) + Om2[k] : (I + ca * Om[k]) + cb * Om2[k];
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (smallT) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - M::cos_(theta)) / theta2;
            B = (theta - M::sin_(theta)) / (theta2 * theta);
        }
    } else {
        C = (o.s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (smallT) {
            A = ((sigma - 1.0) * o.s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * o.s) / (sigma2 * sigma);
        } else {
            const double a = o.s * M::sin_(theta), b = o.s * M::cos_(theta), theta2 = theta * theta, c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    os_quat_from_R(R, o.q);
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + B * Om2[k]) + C * ((k % 4 == 0) ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = (W[3 * i] * u[3] + W[3 * i + 1] * u[4]) + W[3 * i + 2] * u[5];
}

#endif
