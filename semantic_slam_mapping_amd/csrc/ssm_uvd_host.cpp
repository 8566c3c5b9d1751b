// ssm_uvd_host.cpp -- the host half of UVDisparity::Process: the object, and the host-only steps -- the ground line of the V-disparity image, the
// two Kalman filters, and the seeds, flood fills, merge and verification on the U-disparity image.  Small and sequential; the device path (ssm_uvd.hip) runs
// the two steps between its per-pixel phases, ssm_uvd_process_host runs them around the per-pixel stages of include/ssm/uvd_core.h on the CPU.  Plain C++
// without any device call: linked into the library and, as it is, into the CPU sanitizer builds of the host layer (ssm_host.h).
#include "ssm_host.h"
#include <climits>

// GaussianBlur(3 x 3, sigma 0) on u8: the 1-2-1 x 1-2-1 kernel in fixed point, reflect-101 border (a single row / column reflects onto itself)
static void uvd_blur3(const UvdImg& src, int rows, int cols, int stride, UvdImg& dst)
{
    dst.assign((size_t)rows * cols, 0);
    auto at = [&](int r, int c) { if (r < 0) r = rows > 1 ? -r : 0; if (r >= rows) r = rows > 1 ? 2 * rows - 2 - r : 0; if (c < 0) c = cols > 1 ? -c : 0; if (c >= cols) c = cols > 1 ? 2 * cols - 2 - c : 0; return (int)src[(size_t)r * stride + c]; };
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) {
        const int s = at(r - 1, c - 1) + 2 * at(r - 1, c) + at(r - 1, c + 1) + 2 * at(r, c - 1) + 4 * at(r, c) + 2 * at(r, c + 1) + at(r + 1, c - 1) + 2 * at(r + 1, c) + at(r + 1, c + 1);
        dst[(size_t)r * cols + c] = (uint8_t)((s + 8) >> 4);
    }
}
// erode 3 x 3: the minimum over the neighbours inside the image
static void uvd_erode3(const UvdImg& src, int rows, int cols, UvdImg& dst)
{
    dst.assign((size_t)rows * cols, 0);
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) {
        int m = 255;
        for (int dr = -1; dr <= 1; dr++) for (int dc = -1; dc <= 1; dc++) { const int rr = r + dr, cc = c + dc; if (rr >= 0 && rr < rows && cc >= 0 && cc < cols) m = std::min(m, (int)src[(size_t)rr * cols + cc]); }
        dst[(size_t)r * cols + c] = (uint8_t)m;
    }
}
// Otsu: the threshold t that maximises (s1 n2 - s2 n1)^2 / (n1 n2) over the classes {<= t}, {> t}, compared exactly; ascending, the first maximum wins
static int uvd_otsu(const UvdImg& img)
{
    long long hist[256] = {0};
    for (uint8_t v : img) hist[v]++;
    long long N = 0, S = 0;
    for (int i = 0; i < 256; i++) { N += hist[i]; S += (long long)i * hist[i]; }
    unsigned __int128 best_num = 0, best_den = 1; int best = 0;
    long long n1 = 0, s1 = 0;
    for (int t = 0; t < 256; t++) {
        n1 += hist[t]; s1 += (long long)t * hist[t];
        const long long n2 = N - n1, s2 = S - s1;
        if (n1 == 0 || n2 == 0) continue;
        const __int128 a = (__int128)s1 * n2 - (__int128)s2 * n1;
        const unsigned __int128 num = (unsigned __int128)(a * a), den = (unsigned __int128)n1 * (unsigned __int128)n2;
        if (num * best_den > best_num * den) { best_num = num; best_den = den; best = t; }         // num / den > best_num / best_den
    }
    return best;
}

// host step 1 (calVDisparity's sizes, Pitch_Classify's line, Process' Kalman update): F.v_dis holds the h x 256 u8 rows, F.max_disp / min_disp the extremes.
// skip: the frame is not to be run at all
void uvd_host_step1(const ssm_uvd_params& p, UvdKalman& kf1, UvdKalman& kf2, UvdFrame& F, int min_disp, bool skip)
{
    using namespace ssm_uvdc;
    const int h = F.h;
    ssm_uvd_info& I = F.info;
    I = ssm_uvd_info{};
    F.k = FrameK{}; F.k.min_disp = min_disp;
    F.blur.clear(); F.erode.clear(); F.bin.clear(); F.pts.clear(); F.areas.clear(); F.u_raw.clear(); F.u_adj.clear(); F.uni.clear(); F.found.clear(); F.merged.clear(); F.kept.clear();
    I.pitch_filtered = kf1.x;
    if (skip) { I.status = STATUS_SKIPPED; std::fill(F.v_dis.begin(), F.v_dis.end(), 0); return; }
    const int mx = std::max(F.max_disp, 0);
    const int v_cols = (mx + 15) / 16;               // cvCeil(max / 16.0)
    I.v_cols = v_cols; I.u_rows = v_cols + 1; F.k.u_rows = v_cols + 1;
    if (F.max_disp > MAX_RAW) { I.status = STATUS_TOO_LARGE; std::fill(F.v_dis.begin(), F.v_dis.end(), 0); return; }
    for (int r = 0; r < h; r++) for (int c = v_cols; c < MAX_BINS; c++) F.v_dis[(size_t)r * MAX_BINS + c] = 0;       // bin v_cols: the dropped count
    if (v_cols <= 26) { I.status = STATUS_NO_LINE; return; }
    uvd_blur3(F.v_dis, h, v_cols, MAX_BINS, F.blur);
    uvd_erode3(F.blur, h, v_cols, F.erode);
    const int thr = uvd_otsu(F.erode);
    I.otsu_threshold = thr;
    F.bin.resize(F.erode.size());
    for (size_t i = 0; i < F.erode.size(); i++) F.bin[i] = F.erode[i] > thr ? 255 : 0;
    // the point list (uvdisparity.cpp:389-414): per column from 26 on the lowest set pixel, then the set pixels of the 30 rows from it upwards -- it again first
    for (int i = 26; i < v_cols; i++)
        for (int j = h - 1; j >= 0; j--)
            if (F.bin[(size_t)j * v_cols + i] == 255) {
                F.pts.push_back(i); F.pts.push_back(j);
                for (int k = j; k > std::max(j - 30, 0); k--) if (F.bin[(size_t)k * v_cols + i] == 255) { F.pts.push_back(i); F.pts.push_back(k); }
                break;
            }
    const int np = (int)F.pts.size() / 2;
    I.n_line_points = np;
    if (np < 2) { I.status = STATUS_NO_LINE; return; }
    // fitLine(CV_DIST_L2): means and central second moments in double
    double x = 0, y = 0, x2 = 0, y2 = 0, xy = 0;
    for (int i = 0; i < np; i++) { const double px = F.pts[2 * i], py = F.pts[2 * i + 1]; x += px; y += py; x2 += px * px; y2 += py * py; xy += px * py; }
    const double w = np;
    x /= w; y /= w; x2 /= w; y2 /= w; xy /= w;
    const float dx2 = (float)(x2 - x * x), dy2 = (float)(y2 - y * y), dxy = (float)(xy - x * y);
    const float t = (float)atan2((double)(2 * dxy), (double)(dx2 - dy2)) / 2;
    const float line[4] = {(float)cos((double)t), (float)sin((double)t), (float)x, (float)y};
    memcpy(I.line, line, sizeof line);
    const float a = line[0], b = line[1];
    const int x0 = cv_round(line[2]), y0 = cv_round(line[3]);
    const double V_C = y0 - (b / a) * x0;             // float arithmetic, widened (uvdisparity.cpp:447)
    const double theta = atan((p.cv - V_C) / p.f);
    const float z = (float)theta;
    kf1.update(z); kf2.update(z);                     // line2 is fitted to pt_list as well: pitch2 == pitch1
    I.slope = b / a; I.v_c = V_C; I.pitch_measured = z; I.pitch_filtered = kf1.x;
    const double pitch = kf1.x;                       // correct3DPoints(xyz, roi_, pitch1_KF->statePost.at<float>(0), ...)
    F.k.v_c = V_C; F.k.slope = b / a; F.k.cos_p = cos(pitch); F.k.sin_p = sin(pitch); F.k.run = 1;
}

// floodFill(FIXED_RANGE | MASK_ONLY, 8-connected): the 8-connected component of {p : lo <= p <= hi} that contains the seed; returns its pixel count
static int uvd_flood(const UvdImg& img, int rows, int cols, int sr, int sc, int lo, int hi, UvdImg& mask)
{
    mask.assign((size_t)rows * cols, 0);
    std::vector<int> stack; stack.push_back(sr * cols + sc); mask[(size_t)sr * cols + sc] = 255;
    int area = 0;
    while (!stack.empty()) {
        const int at = stack.back(); stack.pop_back(); area++;
        const int r = at / cols, c = at % cols;
        for (int dr = -1; dr <= 1; dr++) for (int dc = -1; dc <= 1; dc++) {
            const int rr = r + dr, cc = c + dc;
            if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
            const size_t q = (size_t)rr * cols + cc;
            if (mask[q] || img[q] < lo || img[q] > hi) continue;
            mask[q] = 255; stack.push_back((int)q);
        }
    }
    return area;
}
static bool uvd_overlap(const UvdImg& a, const UvdImg& b) { for (size_t i = 0; i < a.size(); i++) if (a[i] & b[i]) return true; return false; }

// host step 2 (filterInOut, findAllMasks, mergeMasks, verifyByInliers): F.u_adj is the adjusted U-disparity image, probe_roi / probe_disp what the ROI mask and
// the disparity hold at each match's (v1c, u1c) (a match outside the image: roi 0).  Edits matches / flags as the C ABI describes; F.uni = the union of the kept masks
// record: keep copies of the masks found / merged / kept in F for ssm_debug_uvd_stage (the tests); off, the masks move through the three steps without a copy
void uvd_host_step2(const ssm_uvd_params& p, UvdFrame& F, ssm_pmatch* m, uint8_t* flags, int nm, const uint8_t* probe_roi, const int16_t* probe_disp, bool record)
{
    using namespace ssm_uvdc;
    ssm_uvd_info& I = F.info;
    const int rows = F.k.u_rows, cols = F.w;
    F.uni.assign((size_t)rows * cols, 0);
    // filterInOut (uvdisparity.cpp:68-190)
    const int threshold = -3000;
    for (int i = 0; i < nm; i++) {
        flags[i] &= 1;
        const int uc = (int)m[i].u1c;
        bool keep = probe_roi[i] > 0;
        if (keep && !flags[i]) {
            const double d = std::max(uc - m[i].u2c, 1.0f);
            const double xc = (uc - p.cu) * p.base / d;
            keep = xc > threshold;
        }
        if (keep) m[i].dis_c = probe_disp[i]; else flags[i] |= 2;
    }
    // findAllMasks (uvdisparity.cpp:534-601): the surviving outliers, in order
    UvdImg mask; std::vector<UvdImg> cur;
    for (int i = 0; i < nm; i++) {
        if (flags[i] != 0) continue;
        const int u = (int)m[i].u1c; const short d = m[i].dis_c;
        if (!(d > p.min_disparity_raw)) continue;
        const int dis = cv_round(d / 16.0f);
        if (dis < 0 || dis >= rows || u < 0 || u >= cols) continue;
        const int utense = F.u_adj[(size_t)dis * cols + u];
        if (!(utense > p.min_intense)) continue;
        const int low = 0.5 * utense > p.min_intense ? (int)floor(0.5 * utense) : abs(utense - p.min_intense);
        const int up = 255 - utense;
        const int area = uvd_flood(F.u_adj, rows, cols, dis, u, utense - low, utense + up, mask);
        F.areas.push_back(area);
        if (area > p.min_area) cur.push_back(mask);
    }
    I.n_seeds = (int)F.areas.size(); I.n_masks_found = (int)cur.size();
    if (record) F.found = cur;
    // mergeMasks (uvdisparity.cpp:780-804): a single pass
    for (size_t a = 0; a < cur.size(); a++)
        for (size_t b = a + 1; b < cur.size();) {
            if (uvd_overlap(cur[a], cur[b])) { for (size_t q = 0; q < cur[a].size(); q++) cur[a][q] |= cur[b][q]; cur.erase(cur.begin() + b); }
            else b++;
        }
    I.n_masks_merged = (int)cur.size();
    if (record) F.merged = cur;
    // verifyByInliers (uvdisparity.cpp:680-731)
    std::vector<UvdImg> kept;
    for (UvdImg& k : cur) {
        int num = 0;
        for (int i = 0; i < nm; i++) {
            if (flags[i] != 1) continue;
            const int u = (int)m[i].u1c; const int dis = cv_round(m[i].dis_c / 16.0f);
            if (dis > 0 && dis < rows && u >= 0 && u < cols && k[(size_t)dis * cols + u] != 0) num++;
        }
        if (num < p.inlier_tolerance) kept.push_back(std::move(k));
    }
    I.n_masks_kept = (int)kept.size();
    for (const UvdImg& k : kept) for (size_t q = 0; q < k.size(); q++) F.uni[q] |= k[q];
    if (record) F.kept = std::move(kept);
    if (I.n_masks_kept == 0) F.k.run = 0;
}

// adjustUdisIntense's sigmoid(row, 0.02, 32, 1) per U-disparity row (uvdisparity.cpp:815, :991-996)
static void uvd_rate_table(double* rate) { for (int j = 0; j < ssm_uvdc::MAX_BINS; j++) { const double t = j, scale = 0.02, range = 32; rate[j] = range * 1.0f / (1 + exp(t * scale)); } }


// ---------------------------------------------------------------- the object
extern "C" void ssm_uvd_params_default(ssm_uvd_params* p)
{
    if (!p) return;
    *p = ssm_uvd_params{};
    p->f = 718.8560; p->cu = 607.1928; p->cv = 185.2157; p->base = 0.532331858;         // parameters.txt:37-41
    p->roi_x = 20; p->roi_y = 5; p->roi_z = 40;                                          // :50-54
    p->min_intense = 32; p->min_disparity_raw = 64; p->min_area = 40;                    // USegmentPars()
    p->inlier_tolerance = 3;                                                             // include/track.h:100
}
extern "C" int ssm_uvd_create(ssm_ctx* c, const ssm_uvd_params* params, ssm_uvd** out)
{
    if (!out) return SSM_E_INVAL;
    *out = nullptr;
    if (!params) return host_fail(c, SSM_E_INVAL, "uvd: null parameters");
    if (!(params->f > 0)) return host_fail(c, SSM_E_INVAL, "uvd: the focal length must be positive");
    std::unique_ptr<ssm_uvd> u(new ssm_uvd());
    u->c = c; u->p = *params;
    uvd_rate_table(u->rate);
    if (c) { const int r = uvd_dev_attach(u.get()); if (r) return r; }
    *out = u.release();
    return SSM_OK;
}
extern "C" void ssm_uvd_destroy(ssm_uvd* u)
{
    if (!u) return;
    if (u->c) uvd_dev_release(u);
    delete u;
}
extern "C" int ssm_uvd_reset(ssm_uvd* u)
{
    if (!u) return SSM_E_INVAL;
    const std::unique_lock<std::mutex> lk = host_lock(u->c);
    u->kf1 = UvdKalman(); u->kf2 = UvdKalman();
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_record(ssm_uvd* u, int on) { if (!u) return SSM_E_INVAL; u->record = on != 0; return SSM_OK; }
// the whole of Process on the CPU -- the per-pixel stages from uvd_core.h around the two host steps.  n_matches < 0 skips the frame
extern "C" int ssm_uvd_process_host(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags,
                                    int n_matches, uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info)
{
    if (!u) return SSM_E_INVAL;
    u->frames.resize(1);
    const ssm_uvd_params& p = u->p; const double* rate = u->rate; UvdKalman &kf1 = u->kf1, &kf2 = u->kf2; UvdFrame& F = u->frames[0]; const bool record = u->record;
    using namespace ssm_uvdc;
    if (!left || !disp || w < 1 || h < 1 || h > 32767 || stride < w || (n_matches > 0 && (!matches || !inlier_flags)) || !info) return SSM_E_INVAL;
    const bool skip = n_matches < 0;                 // as nmatch[i] < 0 of ssm_uvd_process_dev
    if (skip) n_matches = 0;
    F.w = w; F.h = h;
    // calVDisparity
    F.v_dis.assign((size_t)h * MAX_BINS, 0);
    int mx = INT_MIN, mn = INT_MAX;
    std::vector<int> cnt(MAX_BINS);
    const float vscale = hist_scale(w);
    for (int i = 0; i < h; i++) {
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int j = 0; j < w; j++) { const short d = disp[(size_t)i * stride + j]; mx = std::max(mx, (int)d); mn = std::min(mn, (int)d); const int b = v_bin(d); if (b >= 0) cnt[b]++; }
        for (int b = 0; b < MAX_BINS; b++) F.v_dis[(size_t)i * MAX_BINS + b] = hist_u8(cnt[b], vscale);
    }
    F.max_disp = mx;
    uvd_host_step1(p, kf1, kf2, F, mn, skip);
    const size_t px = (size_t)w * h;
    std::vector<uint8_t> roi_v(px, 0), ground_v(px, 0), moving_v(px, 0);
    if (F.k.run) {
        const Calib c = uvd_calib(p); const Roi r = uvd_roi(p);
        const int rows = F.k.u_rows;
        std::vector<int> ucnt((size_t)rows * w, 0);
        for (int i = 0; i < h; i++) for (int j = 0; j < w; j++) {
            const short d = disp[(size_t)i * stride + j]; const uint8_t in = left[(size_t)i * stride + j];
            const uint8_t g = ground_pixel(i, d, in, F.k.slope, F.k.v_c), ro = roi_pixel(i, j, d, in, F.k, c, r);
            ground_v[(size_t)i * w + j] = g; roi_v[(size_t)i * w + j] = ro;
            const int b = u_bin(d, ro, g);
            if (b >= 0 && b < rows) ucnt[(size_t)b * w + j]++;
        }
        F.u_raw.resize((size_t)rows * w); F.u_adj.resize((size_t)rows * w);
        const float uscale = hist_scale(h);
        for (int b = 0; b < rows; b++) for (int j = 0; j < w; j++) { const uint8_t raw = hist_u8(ucnt[(size_t)b * w + j], uscale); F.u_raw[(size_t)b * w + j] = raw; F.u_adj[(size_t)b * w + j] = u_adjust(raw, rate[b]); }
        std::vector<uint8_t> pr(n_matches ? n_matches : 1, 0); std::vector<int16_t> pd(n_matches ? n_matches : 1, 0);
        for (int i = 0; i < n_matches; i++) {
            const int uc = (int)matches[i].u1c, vc = (int)matches[i].v1c;
            if (uc >= 0 && uc < w && vc >= 0 && vc < h) { pr[i] = roi_v[(size_t)vc * w + uc]; pd[i] = disp[(size_t)vc * stride + uc]; }
        }
        uvd_host_step2(p, F, matches, inlier_flags, n_matches, pr.data(), pd.data(), record);
        int nmov = 0;
        if (F.k.run)
            for (int i = 0; i < h; i++) for (int j = 0; j < w; j++)
                if (moving_test(disp[(size_t)i * stride + j], roi_v[(size_t)i * w + j], j, F.uni.data(), rows, w)) { moving_v[(size_t)i * w + j] = 255; nmov++; }
        F.info.n_moving = nmov;
    }
    if (roi) memcpy(roi, roi_v.data(), px);
    if (ground) memcpy(ground, ground_v.data(), px);
    if (moving) memcpy(moving, moving_v.data(), px);
    *info = F.info;
    return SSM_OK;
}

// ---------------------------------------------------------------- what the tests look at
extern "C" int ssm_debug_uvd_images(ssm_uvd* u, int frame, uint8_t* v_dis, uint8_t* u_dis, uint8_t* bin, uint8_t* union_mask)
{
    using namespace ssm_uvdc;
    if (!u || frame < 0 || frame >= (int)u->frames.size()) return SSM_E_INVAL;
    const UvdFrame& F = u->frames[frame];
    if (v_dis) memcpy(v_dis, F.v_dis.data(), F.v_dis.size());
    if (u_dis && !F.u_adj.empty()) memcpy(u_dis, F.u_adj.data(), F.u_adj.size());
    if (bin) {
        memset(bin, 0, (size_t)F.h * MAX_BINS);
        if (!F.bin.empty()) for (int r = 0; r < F.h; r++) memcpy(bin + (size_t)r * MAX_BINS, F.bin.data() + (size_t)r * F.info.v_cols, F.info.v_cols);
    }
    if (union_mask && !F.uni.empty()) memcpy(union_mask, F.uni.data(), F.uni.size());
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_times(ssm_uvd* u, double ms[3])
{
    if (!u || !ms) return SSM_E_INVAL;
    for (int i = 0; i < 3; i++) ms[i] = u->call_ms[i];
    return SSM_OK;
}
extern "C" int ssm_debug_uvd_stage(ssm_uvd* u, int frame, int stage, void* out, size_t cap, size_t* bytes)
{
    if (!u || frame < 0 || frame >= (int)u->frames.size() || !bytes) return SSM_E_INVAL;
    const UvdFrame& F = u->frames[frame];
    std::vector<uint8_t> cat;
    const void* src = nullptr; size_t n = 0;
    auto img = [&](const UvdImg& v) { src = v.data(); n = v.size(); };
    auto list = [&](const std::vector<UvdImg>& l) { for (const UvdImg& v : l) cat.insert(cat.end(), v.begin(), v.end()); src = cat.data(); n = cat.size(); };
    if (stage >= 8 && stage <= 10 && !u->record) return SSM_E_INVAL;          // not recorded: ssm_debug_uvd_record
    switch (stage) {
    case 1: img(F.blur); break;
    case 2: img(F.erode); break;
    case 3: img(F.bin); break;
    case 4: src = F.pts.data(); n = F.pts.size() * 4; break;
    case 5: img(F.u_raw); break;
    case 7: src = F.areas.data(); n = F.areas.size() * 4; break;
    case 8: list(F.found); break;
    case 9: list(F.merged); break;
    case 10: list(F.kept); break;
    default: return SSM_E_INVAL;
    }
    *bytes = n;
    if (!out) return SSM_OK;
    if (n > cap) return SSM_E_CAPACITY;
    if (n) memcpy(out, src, n);
    return SSM_OK;
}
