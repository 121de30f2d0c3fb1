// orbx_normal_depth.h -- the arithmetic of MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:477-521) on the project's OpenCV stand-in
// (oracle/cvshim/cvshim.hpp:411-418, 480-492), operation by operation, as device functions: shared by orbx_mappoint.hip (orbx_mappoint_refresh)
// and orbx_loop_correct.hip (the refresh of a point that LoopClosing::CorrectLoop has just moved).  Every product, sum and quotient is its own
// IEEE operation (-ffp-contract=off; f64 sqrt and division are IEEE).
#ifndef ORBX_NORMAL_DEPTH_H
#define ORBX_NORMAL_DEPTH_H

#include <hip/hip_runtime.h>
#include <math.h>

// u = (pos - Ow) / |pos - Ow|: v in float, the norm accumulated in double from 0, the quotient in double, narrowed
__device__ __forceinline__ void mp_unit(const float *__restrict__ pos, const float *__restrict__ ow, float *u)
{
    const float v0 = pos[0] - ow[0], v1 = pos[1] - ow[1], v2 = pos[2] - ow[2];
    double s = 0.0;
    s = s + (double)v0 * (double)v0;
    s = s + (double)v1 * (double)v1;
    s = s + (double)v2 * (double)v2;
    s = sqrt(s);
    u[0] = (float)((double)v0 / s); u[1] = (float)((double)v1 / s); u[2] = (float)((double)v2 / s);
}

// component c of normal / n: the float sum of the unit vectors SEQUENTIALLY in list order (a float sum of three or more terms depends on the
// order: nothing is tree-reduced), then the double quotient, narrowed
__device__ __forceinline__ float mp_normal_component(const float *unit, int n, int c)
{
    float acc = 0.0f;
    for (int o = 0; o < n; o++) acc = acc + unit[o * 3 + c];
    return (float)((double)acc / (double)n);
}

// dist = (float)|pos - refOw|, mfMaxDistance = dist * refScale, mfMinDistance = mfMaxDistance / topScale
__device__ __forceinline__ void mp_depth(const float *pos, const float *refc, float refScale, float topScale, float *maxD, float *minD)
{
    const float v0 = pos[0] - refc[0], v1 = pos[1] - refc[1], v2 = pos[2] - refc[2];
    double s = 0.0;
    s = s + (double)v0 * (double)v0;
    s = s + (double)v1 * (double)v1;
    s = s + (double)v2 * (double)v2;
    const float dist = (float)sqrt(s);
    const float mx = dist * refScale;
    *maxD = mx;
    *minD = mx / topScale;
}

#endif
