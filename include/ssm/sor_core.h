// sor_core.h -- the arithmetic of the statistical outlier removal (pcl::StatisticalOutlierRemoval as reference src/mapper.cpp:137-146 would use it, were the block
// not commented out there), compiled for host and device like motion_fuse_core.h and uvd_core.h: csrc/kernels_sor.hip and the host function of
// csrc/ssm_sor_host.cpp call the same functions, so device == host bit for bit.  Every translation unit that includes this is built with
// -ffp-contract=off.  What is here: the squared distance, the mean of a point's k smallest, the exact integer statistics and the threshold they give, and the
// geometry of the search ladder (cell function, key, settle bound, plan), which decides how fast a point's k nearest are found and never which they are.
#pragma once
#include <stdint.h>
#include <math.h>
#include <float.h>
#if defined(__HIPCC__)
#define SOR_HD __host__ __device__ inline
#else
#define SOR_HD inline
#endif

namespace ssm_sorc {

static const int MAX_K = 64;                   // one best per lane of a wave on the device; the host function keeps the same limit
static const int CHUNK = 512;                  // candidates per LDS chunk of the device search (ssm_sor_chunk): a candidate list of any length streams through it
static const int AXIS_BITS = 21;               // cells per axis that a key holds: key = z << 42 | y << 21 | x, so the three x-neighbours are adjacent keys
static const int MAX_LEVELS = 24;              // after the plan has raised c0 the top level is at most AXIS_BITS - 1
static const uint64_t KEY_NONE = ~(uint64_t)0; // a point that takes no part (non-finite): behind every cell in key order
static const float D_LIMIT = 4096.0f;          // the statistics grid: 2^-20 m steps below 4096 m, so q < 2^32 and q * q fits 64 bits
static const double Q_SCALE = 1048576.0;

SOR_HD bool finite1(float v) { return fabsf(v) <= FLT_MAX; }          // false for NaN
SOR_HD bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }

// FLANN's L2_Simple on floats: float differences, (dx^2 + dy^2) + dz^2
SOR_HD float dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
// the k smallest squared distances in ascending order: dist_sum += root(d2) in double, in that order; d_i = mean_of(dist_sum, k)
SOR_HD double root(float d2) { return sqrt((double)d2); }
SOR_HD float mean_of(double dist_sum, int k) { return (float)(dist_sum / (double)k); }

// the exact statistics: d_i goes ONCE onto the grid (half-even), and S1 = sum q, S2 = sum q^2 as sum of its low and of its high 32 bits, all in u64
SOR_HD bool on_grid(float d) { return d < D_LIMIT; }                  // d >= 0 or NaN / inf: those are off the grid
SOR_HD uint64_t quantise(float d) { return (uint64_t)llrint((double)d * Q_SCALE); }
struct Stats { double mean, stddev, threshold; };
// host only: the one place the threshold's sqrt is evaluated; the device path reads the three integers down and calls this
inline Stats stats_of(int64_t n, uint64_t s1, uint64_t s2_lo, uint64_t s2_hi, double stddev_mul)
{
    const double a = (double)s1 * (1.0 / Q_SCALE);
    const double b = ((double)s2_hi * 4294967296.0 + (double)s2_lo) * (1.0 / Q_SCALE) * (1.0 / Q_SCALE);
    Stats s;
    s.mean = a / (double)n;
    const double variance = (b - a * a / (double)n) / (double)(n - 1);
    s.stddev = sqrt(variance > 0.0 ? variance : 0.0);
    s.threshold = s.mean + stddev_mul * s.stddev;
    return s;
}
SOR_HD bool keeps(float d, double threshold) { return (double)d <= threshold; }

// ---- the ladder.  Level l has cells of c = c0 * 2^l (exact in double).  The cell of a coordinate is computed in double, so its relative error is below 2^-51
// and two points whose cell indices differ by at least 2 on an axis are farther apart than c (1 - 2^-30) in exact arithmetic, hence than c (1 - 2^-20) in the float
// arithmetic of dist2.  A point that has seen k others in the 27 cells around its own and whose k-th squared distance is <= settle_r2(c) = (c (1 - 2^-10))^2 can
// therefore not have a nearer neighbour outside them.
SOR_HD double cell_of(float v, float lo, double c) { return floor(((double)v - (double)lo) / c); }          // >= 0 for v >= lo
SOR_HD double level_cell(float c0, int level) { return (double)c0 * (double)((uint64_t)1 << level); }
SOR_HD float settle_r2(double c) { const float r = (float)c * 0.9990234375f; return r * r; }
SOR_HD uint64_t key_of(int64_t cx, int64_t cy, int64_t cz) { return ((uint64_t)cz << (2 * AXIS_BITS)) | ((uint64_t)cy << AXIS_BITS) | (uint64_t)cx; }
SOR_HD uint64_t point_key(float x, float y, float z, const float lo[3], double c)
{
    return key_of((int64_t)cell_of(x, lo[0], c), (int64_t)cell_of(y, lo[1], c), (int64_t)cell_of(z, lo[2], c));
}
// the nine runs of keys that cover the 27 cells around (cx, cy, cz): run r = (dy, dz) = (r % 3 - 1, r / 3 - 1) -> keys [first, last], or false when it lies outside the grid
SOR_HD bool key_run(int64_t cx, int64_t cy, int64_t cz, int r, uint64_t* first, uint64_t* last)
{
    const int64_t top = ((int64_t)1 << AXIS_BITS) - 1, y = cy + (r % 3 - 1), z = cz + (r / 3 - 1);
    if (y < 0 || y > top || z < 0 || z > top) return false;
    *first = key_of(cx > 0 ? cx - 1 : 0, y, z); *last = key_of(cx < top ? cx + 1 : top, y, z);
    return true;
}

// host only: what the bounding box of the finite points, the caller's cell (0: automatic) and n fix of the ladder.  c0 is doubled until the box fits the key's
// bits; `top` is the first level at which the box spans at most three cells per axis -- there every point is a candidate of every other, so the ladder ends.
struct Plan { float lo[3], hi[3], c0; int top; };
inline double plan_span(const Plan& p, double c)          // the largest cell index of the box
{
    double m = 0.0;
    for (int a = 0; a < 3; a++) { const double v = cell_of(p.hi[a], p.lo[a], c); if (v > m) m = v; }
    return m;
}
inline Plan plan_of(const float lo[3], const float hi[3], float cell, int64_t n_finite)
{
    Plan p;
    double ext = 0.0;
    for (int a = 0; a < 3; a++) { p.lo[a] = lo[a]; p.hi[a] = hi[a]; const double e = (double)hi[a] - (double)lo[a]; if (e > ext) ext = e; }
    // automatic: a quarter of the spacing n points would have on a plane of the box's size -- depth clouds are surfaces, and several times denser near the camera
    p.c0 = cell > 0.0f ? cell : (float)(0.25 * ext / sqrt((double)(n_finite > 0 ? n_finite : 1)));
    if (!(p.c0 > 0.0f) || !finite1(p.c0)) p.c0 = 1.0f;
    while (plan_span(p, (double)p.c0) > (double)(((int64_t)1 << AXIS_BITS) - 1) && finite1(p.c0 * 2.0f)) p.c0 *= 2.0f;
    p.top = 0;
    while (p.top < MAX_LEVELS - 1 && plan_span(p, level_cell(p.c0, p.top)) > 2.0) p.top++;
    return p;
}

}      // namespace ssm_sorc
