// kernels_relabel.hip -- label fusion of one cloud in device memory under up to 16 views: every point's twelve counters, its new label and the
// info counts.  The arithmetic is include/ssm/relabel_core.h, which the host function of ssm_relabel_host.cpp calls too.
//
// One thread per point.  The view records (two pointers, carve_core.h's Setup, 12 doubles: 192 bytes each) are the same in every lane: they come as a kernel
// argument, so a view's record is read by scalar loads, once per wave.  The twelve counters are one 64-bit value in registers.  What goes out per point is its
// record (8 + 4 bytes, for ssm_debug_relabel_record and the host-array call) and, for a changed point only, the 4 label bytes of the cloud.  The info counts go
// per wave (ballots; the two pair counts by a wave reduction), per block through LDS, then one integer atomic per non-zero count and block.
// The time is the gathers, up to v (2 r + 1)^2 pixels per point at addresses that differ per lane; the packed form halves their number, and with the windows of two views
// in flight before either is judged it won on an MI355X (profiles/r22_relabel.md): that is the default, the other two stay behind ssm_debug_relabel_form.
// No floating-point atomic, no grid barrier, no block waits for another.
#include "ssm_internal.h"
#include "../../include/ssm/relabel_core.h"
#include "../../include/ssm/render_core.h"
using namespace ssm_relabelc;

#define RELABEL_T 256
#define RELABEL_W (RELABEL_T / 64)
#define RELABEL_NCOUNT 6          // n_supported, n_voted, n_changed, n_filled, pairs_supported, pairs_voted

// a wave's sum of a small non-negative value (at most 2^16 / 64 per lane here)
__device__ inline int relabel_wave_sum(int v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- the packed forms: the views' images are one uint32 per pixel, depth | label << 16 (View::depth points at it, View::label is unused) -- one gather stream
// instead of two.  s.16 steps 1-7 and s.20 step 2 restated over the packed image in three pieces -- the same operations in the same order as carve_core.h
// verdict_at and relabel_core.h view_vote, with the window read once for both the depth minimum and the label guard
struct RelabelProj { bool ok; int px, py; double qz; };
// s.16 steps 1-4: the pixel, or ok = false (the verdict is UNKNOWN)
__device__ inline RelabelProj relabel_project(float xf, float yf, float zf, const View& V)
{
    using namespace ssm_carvec;
    const Setup& S = V.S; const double* M = V.M;
    RelabelProj P{false, 0, 0, 0.0};
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    if (!(finite_d(x) && finite_d(y) && finite_d(z))) return P;
    const double qx = M[0] * x + M[1] * y + M[2] * z + M[3];
    const double qy = M[4] * x + M[5] * y + M[6] * z + M[7];
    const double qz = M[8] * x + M[9] * y + M[10] * z + M[11];
    if (!(finite_d(qx) && finite_d(qy) && finite_d(qz)) || qz < S.z_min) return P;
    const double u = S.fx * (qx / qz) + S.cx, v = S.fy * (qy / qz) + S.cy;
    const double pxd = floor(u + 0.5), pyd = floor(v + 0.5);
    const double r = (double)S.r;
    if (!(pxd >= r && pxd <= (double)(S.w - 1) - r && pyd >= r && pyd <= (double)(S.h - 1) - r)) return P;
    P.ok = true; P.px = (int)pxd; P.py = (int)pyd; P.qz = qz;
    return P;
}
// s.16 steps 5-7 and the vote, from the centre pixel, the window's minimum and whether the whole window carries the centre's label
__device__ inline uint64_t relabel_judge(uint64_t c, const View& V, const RelabelProj& P, uint32_t centre, int32_t dmin, bool same, int edge_guard, int* supported, int* voted)
{
    using namespace ssm_carvec;
    const Setup& S = V.S;
    *supported = 0; *voted = 0;
    if (!P.ok || dmin == 0) return c;
    const int64_t d = (int64_t)(centre & 0xffffu);
    const double zs = P.qz * S.scale;
    const int64_t zq = zs < ZQ_LIMIT ? (int64_t)llrint(zs) : (int64_t)ZQ_LIMIT;
    const int64_t tol = S.tol_abs + (d * S.ppm) / 1000000;
    if (zq + tol < (int64_t)dmin) return c;
    const int64_t diff = zq > d ? zq - d : d - zq;
    if (!(diff <= tol)) return c;
    *supported = 1;
    const uint32_t l = centre >> 16;
    if (l >= (uint32_t)N_LABELS) return c;
    if (edge_guard && !same) return c;
    *voted = 1;
    return c + one_of(l);
}
__device__ inline const uint32_t* relabel_window(const View& V, const RelabelProj& P)          // the window's first pixel (an inside pixel always: P.ok)
{
    return reinterpret_cast<const uint32_t*>(V.depth) + (size_t)(P.py - V.S.r) * (size_t)V.S.w + (size_t)(P.px - V.S.r);
}
// one view: the view loop as written
__device__ inline uint64_t relabel_vote_packed(uint64_t c, float x, float y, float z, const View& V, int edge_guard, int* supported, int* voted)
{
    const RelabelProj P = relabel_project(x, y, z, V);
    uint32_t centre = 0; int32_t dmin = 65536; bool same = true;
    if (P.ok) {
        const int r = V.S.r, n = 2 * r + 1;
        const uint32_t* win = relabel_window(V, P);
        centre = win[(size_t)r * (size_t)V.S.w + (size_t)r];
        for (int dy = 0; dy < n; dy++) {
            const uint32_t* row = win + (size_t)dy * (size_t)V.S.w;
            for (int dx = 0; dx < n; dx++) { const uint32_t e = row[dx]; const int32_t d = (int32_t)(e & 0xffffu); dmin = d < dmin ? d : dmin; same = same && (e >> 16) == (centre >> 16); }
        }
    }
    return relabel_judge(c, V, P, centre, dmin, same, edge_guard, supported, voted);
}
// two views in flight: both are projected first, then ONE loop walks both windows, so the gathers of the two views are issued side by side before either view
// is judged.  A view without a pixel loads nothing.  The radius is the call's, the same in both views; the counters take the votes in view order
__device__ inline uint64_t relabel_vote_pair(uint64_t c, float x, float y, float z, const View& VA, const View& VB, int edge_guard, int* supported, int* voted)
{
    const RelabelProj PA = relabel_project(x, y, z, VA), PB = relabel_project(x, y, z, VB);
    const int r = VA.S.r, n = 2 * r + 1;
    const uint32_t* wa = PA.ok ? relabel_window(VA, PA) : nullptr;
    const uint32_t* wb = PB.ok ? relabel_window(VB, PB) : nullptr;
    const uint32_t ca = PA.ok ? wa[(size_t)r * (size_t)VA.S.w + (size_t)r] : 0u, cb = PB.ok ? wb[(size_t)r * (size_t)VB.S.w + (size_t)r] : 0u;
    int32_t mina = 65536, minb = 65536; bool sa = true, sb = true;
    for (int dy = 0; dy < n; dy++) {
        for (int dx = 0; dx < n; dx++) {
            const uint32_t ea = PA.ok ? wa[(size_t)dy * (size_t)VA.S.w + (size_t)dx] : 0xffffu, eb = PB.ok ? wb[(size_t)dy * (size_t)VB.S.w + (size_t)dx] : 0xffffu;
            const int32_t da = (int32_t)(ea & 0xffffu), db = (int32_t)(eb & 0xffffu);
            mina = da < mina ? da : mina; minb = db < minb ? db : minb;
            sa = sa && (ea >> 16) == (ca >> 16); sb = sb && (eb >> 16) == (cb >> 16);
        }
    }
    int s0, t0, s1, t1;
    c = relabel_judge(c, VA, PA, ca, mina, sa, edge_guard, &s0, &t0);
    c = relabel_judge(c, VB, PB, cb, minb, sb, edge_guard, &s1, &t1);
    *supported = s0 + s1; *voted = t0 + t1;
    return c;
}

template <int FORM> __global__ void __launch_bounds__(RELABEL_T)
relabel_kernel(const RelabelArgs A, ssm_point* __restrict__ pts, int n, uint64_t* __restrict__ votes, uint32_t* __restrict__ new_label, unsigned long long* __restrict__ info)
{
    __shared__ int cnt_s[RELABEL_W][RELABEL_NCOUNT];
    const int i = blockIdx.x * RELABEL_T + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = i < n;
    int ns = 0, nv = 0; bool changed = false, filled = false;
    if (live) {
        const float4 q = *reinterpret_cast<const float4*>(pts + i);
        const uint32_t L0 = pts[i].label;
        uint64_t c = own_vote(L0, A.own_weight);
        int k = 0;
        if (FORM == RELABEL_FORM_PAIRS) for (; k + 1 < A.v; k += 2) { int s, t; c = relabel_vote_pair(c, q.x, q.y, q.z, A.view[k], A.view[k + 1], A.edge_guard, &s, &t); ns += s; nv += t; }
        for (; k < A.v; k++) {
            int s, t;
            c = FORM == RELABEL_FORM_IMAGES ? view_vote(c, q.x, q.y, q.z, A.view[k], A.edge_guard, &s, &t) : relabel_vote_packed(c, q.x, q.y, q.z, A.view[k], A.edge_guard, &s, &t);
            ns += s; nv += t;
        }
        const uint32_t L1 = decide(L0, c, A.min_votes);
        votes[i] = c; new_label[i] = L1;
        changed = L1 != L0; filled = changed && L0 >= (uint32_t)N_LABELS;
        if (changed) pts[i].label = L1;
    }
    const int c0 = __popcll(__ballot(ns > 0)), c1 = __popcll(__ballot(nv > 0)), c2 = __popcll(__ballot(changed)), c3 = __popcll(__ballot(filled));
    const int pairs = relabel_wave_sum(ns | nv << 16);          // 64 lanes x 16 views at most: each half stays below 2^16
    if (lane == 0) { int* w = cnt_s[wave]; w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3; w[4] = pairs & 0xffff; w[5] = pairs >> 16; }
    __syncthreads();
    if (threadIdx.x < RELABEL_NCOUNT) {
        int t = 0;
        for (int w = 0; w < RELABEL_W; w++) t += cnt_s[w][threadIdx.x];
        if (t) atomicAdd(info + threadIdx.x, (unsigned long long)t);
    }
}

// a view's images from what the host uploaded: the label image of the semantic BGR image and, for the packed form, depth | label << 16
__global__ void __launch_bounds__(RELABEL_T)
relabel_labels_kernel(const uint8_t* __restrict__ bgr, const uint16_t* __restrict__ depth, int64_t np, uint8_t* __restrict__ label, uint32_t* __restrict__ packed)
{
    const int64_t i = (int64_t)blockIdx.x * RELABEL_T + threadIdx.x;
    if (i >= np) return;
    const uint8_t* p = bgr + 3 * i;
    const uint8_t l = ssm_renderc::label_of_bgr24((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
    label[i] = l;
    if (packed) packed[i] = (uint32_t)depth[i] | (uint32_t)l << 16;
}

// ------------------------------------------------------------------ launchers
hipError_t k_relabel_labels(const uint8_t* bgr, const uint16_t* depth, int64_t np, uint8_t* label, uint32_t* packed, hipStream_t s)
{
    if (np > 0) relabel_labels_kernel<<<(unsigned)((np + RELABEL_T - 1) / RELABEL_T), RELABEL_T, 0, s>>>(bgr, depth, np, label, packed);
    return hipGetLastError();
}
// info: RELABEL_NCOUNT counts, cleared here; votes, new_label: n entries.  Queues everything on s and waits for nothing
hipError_t k_relabel(const RelabelArgs& A, int form, ssm_point* pts, int n, uint64_t* votes, uint32_t* new_label, unsigned long long* info, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(info, 0, RELABEL_NCOUNT * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (n > 0) {
        const unsigned nb = (unsigned)((n + RELABEL_T - 1) / RELABEL_T);
        if (form == RELABEL_FORM_PAIRS) relabel_kernel<RELABEL_FORM_PAIRS><<<nb, RELABEL_T, 0, s>>>(A, pts, n, votes, new_label, info);
        else if (form == RELABEL_FORM_PACKED) relabel_kernel<RELABEL_FORM_PACKED><<<nb, RELABEL_T, 0, s>>>(A, pts, n, votes, new_label, info);
        else relabel_kernel<RELABEL_FORM_IMAGES><<<nb, RELABEL_T, 0, s>>>(A, pts, n, votes, new_label, info);
    }
    return hipGetLastError();
}
