// prior_math.hpp: a geometric prior of the tracker - 9 float64 values P (row-major) that map reference pixel coordinates to monitored
// pixel coordinates - as plain C++ on doubles, shared by the seeded LK kernels (k_lk2.hip: the start position of every key point), the
// mask kernel (k_prior.hip), the host form of its launcher (k_prior.hpp) and, transcribed, tests/lk_prior_restatement.py, which is the
// definition.  Every operation rounds on its own, in the order written: this text needs -ffp-contract=off and a
// correctly rounded division on every compiler that reads it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_HD __host__ __device__
#else
#define PM_HD
#endif

namespace pm {

// (x, y) of a tile at (x_off, y_off) -> (qx, qy) in the same tile's coordinates.  false: the row has no guess (w not finite or <= 0)
PM_HD inline bool map(const double *P, double x_off, double y_off, double x, double y, double &qx, double &qy)
{
    const double gx = x + x_off, gy = y + y_off;
    const double w = (P[6] * gx + P[7] * gy) + P[8];
    if (!(w > 0.0) || !(w < INFINITY)) return false;
    qx = ((P[0] * gx + P[1] * gy) + P[2]) / w;
    qy = ((P[3] * gx + P[4] * gy) + P[5]) / w;
    qx = qx - x_off;
    qy = qy - y_off;
    return true;
}

// the tracker's start position of a key point: the float32 of the mapped position
PM_HD inline bool guess(const double *P, double x_off, double y_off, float px, float py, float &gx, float &gy)
{
    double qx, qy;
    if (!map(P, x_off, y_off, (double)px, (double)py, qx, qy)) return false;
    gx = (float)qx; gy = (float)qy;
    return true;
}

// the monitored pixel a reference pixel is held against (rule 4): (qx, qy) rounded half to even, inside a W x H box.  The comparisons
// run on the rounded doubles: a position that is not finite or far outside never reaches the cast
PM_HD inline bool target(const double *P, double x_off, double y_off, int x, int y, int W, int H, int &rx, int &ry)
{
    double qx, qy;
    if (!map(P, x_off, y_off, (double)x, (double)y, qx, qy)) return false;
    const double fx = rint(qx), fy = rint(qy);
    if (!(fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H)) return false;
    rx = (int)fx; ry = (int)fy;
    return true;
}

// one image's half of the automatic mask (the reference's klt.py:268-273): not 0, finite, not the nodata value
template <typename T> PM_HD inline bool valid(T v, int has_nodata, double nodata)
{
    bool ok = v != (T)0;
    if ((T)0.5 != (T)0) ok = ok && ((double)v - (double)v == 0.0);      // (floating types: finite)
    if (has_nodata) ok = ok && ((double)v != nodata);
    return ok;
}

}  // namespace pm
