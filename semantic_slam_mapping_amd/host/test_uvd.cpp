// test_uvd -- the U/V-disparity moving-object stage through the C++ host classes (run by tests/test_gpu_uvd_host.py under -m gpu): Tracker with uv_disparity=1
// (UVDisparity::Process after every successful stereo VO) against BatchStereoTracker (one ssm_uvd_process_dev per chunk) on a KITTI-layout stereo sequence
// (argv[2]): same masks and pitches with a chunk size that splits the sequence; with uv_disparity=0 both behave as before -- empty masks, the same poses.
// Prints one "PASS name" / "FAIL name" line per check; exit code = number of failures.
//
// Without a sequence directory (`test_uvd` or `test_uvd <parameters>`) it runs the host-only checks: class UVDisparity on a thread without a device context takes
// ssm_uvd_process_host -- no device call, so this half runs in the CPU suite and, built with -DSSM_UVD_HOST_ONLY against host/san_stub_device.cpp and the
// library's own host sources, under the sanitizers.
#include "ssm/uvdisparity.hpp"
#ifndef SSM_UVD_HOST_ONLY
#include "ssm/rgbdframe.h"
#include "ssm/track.h"
#include "ssm/batch_stereo_tracker.h"
using namespace rgbd_tutor;
#endif
using namespace std;
static int fails = 0;
#define CHECK(name, cond) do { if (cond) cout << "PASS " << name << endl; else { cout << "FAIL " << name << endl; fails++; } } while (0)

// a 160 x 96 scene: ground d(v) = v - 40 below the horizon, a box of disparity 40 on columns 56 .. 103 from row 30 down to the ground, a few holes; the left image
// is a seeded pattern with some zero pixels.  Outliers sit on the box, inliers on the ground
static int host_checks()
{
    const int W = 160, H = 96;
    cv::Mat left(H, W, CV_8UC1), disp(H, W, CV_16SC1), xyz, roi, ground;
    uint32_t lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; };
    for (int v = 0; v < H; v++) for (int u = 0; u < W; u++) {
        int d = v > 40 ? 16 * (v - 40) + (int)(rnd() % 3) - 1 : -16;
        if (u >= 56 && u < 104 && v >= 30 && v <= 80) d = 16 * 40 + (int)(rnd() % 3) - 1;
        if ((u / 7 + v / 5) % 23 == 0) d = -16;
        disp.at<int16_t>(v, u) = (int16_t)d;
        left.at<uchar>(v, u) = (uchar)(rnd() % 97 == 0 ? 0 : 1 + rnd() % 255);
    }
    VisualOdometryStereo::parameters vp; vp.calib.f = 100; vp.calib.cu = 80.3; vp.calib.cv = 40; vp.base = 1.0;
    VisualOdometryStereo vo(vp);
    auto add = [&](vector<pmatch>& list, int u, int v) {
        pmatch m; memset(static_cast<void*>(&m), 0, sizeof m);
        const float d = max((int)disp.at<int16_t>(v, u), 16) / 16.0f;
        m.u1c = (float)u; m.v1c = (float)v; m.u2c = u - d; m.v2c = (float)v; m.u1p = u + 1.0f; m.v1p = (float)v; m.u2p = u + 1.0f - d; m.v2p = (float)v;
        list.push_back(m);
    };
    auto fill = [&]() {
        vo.quadmatches_inlier.clear(); vo.quadmatches_outlier.clear();
        add(vo.quadmatches_outlier, 70, 35); add(vo.quadmatches_outlier, 90, 45); add(vo.quadmatches_outlier, 5, 3);        // the last one: above the horizon, outside the ROI mask
        add(vo.quadmatches_inlier, 20, 85); add(vo.quadmatches_inlier, 140, 90); add(vo.quadmatches_inlier, 150, 2);
    };
    fill();
    CalibPars calib(100, 80.3, 40, 1.0); ROI3D r3(20, 5, 40);
    UVDisparity uv;
    uv.SetCalibPars(calib); uv.SetROI3D(r3); uv.SetOutThreshold(6.0f); uv.SetInlierTolerance(3); uv.SetMinAdjustIntense(20); uv.SetUSegmentPars(32, 64, 40);
    double p1 = -1, p2 = -2;
    cv::Mat moving = uv.Process(left, disp, vo, xyz, roi, ground, p1, p2);
    long nmov = 0, nroi = 0, ngr = 0;
    for (int v = 0; v < H; v++) for (int u = 0; u < W; u++) { nmov += moving.at<uchar>(v, u) == 255; nroi += roi.at<uchar>(v, u) > 0; ngr += ground.at<uchar>(v, u) > 0; }
    const ssm_uvd_info i1 = uv.last_info;
    CHECK("uvd_host_class_runs_without_a_device", !uv.onDevice() && i1.status == 0 && i1.v_cols > 26 && i1.n_line_points >= 2);
    CHECK("uvd_host_class_fills_the_masks", moving.rows == H && moving.cols == W && roi.rows == H && ground.cols == W && nmov > 0 && nmov == i1.n_moving && nroi > nmov && ngr > 0 && xyz.empty());
    CHECK("uvd_host_class_edits_the_vo_lists", vo.quadmatches_outlier.size() == 2 && vo.quadmatches_inlier.size() == 2 && vo.quadmatches_outlier[0].dis_c == disp.at<int16_t>(35, 70) &&
          vo.quadmatches_inlier[1].dis_c == disp.at<int16_t>(90, 140));
    CHECK("uvd_host_class_pitches", p1 == p2 && p1 == (double)i1.pitch_measured && i1.n_masks_kept >= 1);
    // the C function directly, on a fresh object: the same bits; a second frame through the class moves the Kalman filter, not the measurement
    ssm_uvd_params P; ssm_uvd_params_default(&P);
    P.f = 100; P.cu = 80.3; P.cv = 40; P.base = 1.0; P.roi_x = 20; P.roi_y = 5; P.roi_z = 40;
    ssm_uvd* u = nullptr; ssm_uvd_info i2; vector<uint8_t> m2((size_t)W * H), r2((size_t)W * H), g2((size_t)W * H);
    bool direct = ssm_uvd_create(nullptr, &P, &u) == SSM_OK;
    fill();
    vector<ssm_pmatch> qm; vector<uint8_t> fl;
    for (const pmatch& q : vo.quadmatches_inlier) { ssm_pmatch t; memcpy(&t, &q, sizeof t); qm.push_back(t); fl.push_back(1); }
    for (const pmatch& q : vo.quadmatches_outlier) { ssm_pmatch t; memcpy(&t, &q, sizeof t); qm.push_back(t); fl.push_back(0); }
    direct = direct && ssm_uvd_process_host(u, left.data, disp.ptr<int16_t>(), W, H, W, qm.data(), fl.data(), (int)qm.size(), m2.data(), r2.data(), g2.data(), &i2) == SSM_OK;
    direct = direct && memcmp(&i1, &i2, sizeof i1) == 0 && memcmp(m2.data(), moving.data, m2.size()) == 0 && memcmp(r2.data(), roi.data, r2.size()) == 0 && memcmp(g2.data(), ground.data, g2.size()) == 0;
    direct = direct && fl[2] == 3 && fl[5] == 2 && fl[0] == 1 && fl[3] == 0;
    ssm_uvd_destroy(u);
    CHECK("uvd_host_class_equals_the_c_function", direct);
    // the same ssm_uvd_create with and without a device: it refuses a focal length that is not positive
    P.f = 0; u = nullptr;
    CHECK("uvd_create_refuses_a_focal_length_of_zero", ssm_uvd_create(nullptr, &P, &u) == SSM_E_INVAL && u == nullptr && string(ssm_last_error(nullptr)) == "uvd: the focal length must be positive");
    uv.Process(left, disp, vo, xyz, roi, ground, p1, p2);
    CHECK("uvd_host_class_keeps_its_kalman_state", uv.last_info.pitch_measured == i1.pitch_measured && uv.last_info.pitch_filtered != i1.pitch_filtered);
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
#ifdef SSM_UVD_HOST_ONLY
int main() { return host_checks(); }
#else

struct Run { vector<Eigen::Isometry3d> T; vector<cv::Mat> moving, roi, ground; vector<double> pitch; vector<int> ran; };
static bool same_mat(const cv::Mat& a, const cv::Mat& b)
{
    if (a.empty() || b.empty()) return a.empty() && b.empty();
    return a.rows == b.rows && a.cols == b.cols && memcmp(a.data, b.data, (size_t)a.rows * a.cols) == 0;
}
int main(int argc, char** argv)
{
    if (argc < 3) return host_checks();
    ParameterReader para(argv[1]);
    para.set("data_source", argv[2]); para.set("start_index", "0"); para.set("end_index", "100"); para.set("tracker_mode", "stereo");
    para.set("image_width", "400"); para.set("image_height", "120"); para.set("orb_levels", "3"); para.set("orb_features", "300");
    para.set("camera.baseline", "0.532331858"); para.set("camera.roix", "2000"); para.set("camera.roiy", "2000"); para.set("camera.roiz", "4000");
    VisualOdometryStereo::parameters vp; vp.calib.f = para.getData<double>("camera.fx"); vp.calib.cu = para.getData<double>("camera.cx"); vp.calib.cv = para.getData<double>("camera.cy");
    vp.base = 0.532331858; vp.inlier_threshold = 2.0;
    Run per[2], bulk[2];
    for (int uv = 0; uv < 2; uv++) {
        para.set("uv_disparity", uv ? "1" : "0");
        {
            para.set("kitti_reader_depth", "1");
            Tracker tracker(para, vp); FrameReader rd(para, FrameReader::KITTI);
            while (RGBDFrame::Ptr f = rd.next()) {
                tracker.updateFrame(f);
                per[uv].T.push_back(f->getTransform()); per[uv].moving.push_back(f->moving_mask); per[uv].roi.push_back(f->roi_mask); per[uv].ground.push_back(f->ground_mask);
                per[uv].ran.push_back(!f->moving_mask.empty()); per[uv].pitch.push_back(f->moving_mask.empty() ? 0.0 : tracker.pitch1);
            }
        }
        {
            para.set("kitti_reader_depth", "0");
            FrameReader rd(para, FrameReader::KITTI);
            BatchStereoTracker bs(para, vp, 400, 120, 4);            // chunks of 4: the 6 frames are split, the Kalman filters run across the border
            auto take = [&](const vector<RGBDFrame::Ptr>& done) {
                for (size_t i = 0; i < done.size(); i++) {
                    bulk[uv].T.push_back(done[i]->getTransform()); bulk[uv].moving.push_back(done[i]->moving_mask); bulk[uv].roi.push_back(done[i]->roi_mask); bulk[uv].ground.push_back(done[i]->ground_mask);
                    bulk[uv].ran.push_back(bs.infos[i].uv); bulk[uv].pitch.push_back(bs.infos[i].pitch1);
                }
            };
            while (RGBDFrame::Ptr f = rd.next()) take(bs.push(f));
            take(bs.flush());
            para.set("kitti_reader_depth", "1");
        }
    }
    const size_t n = per[1].T.size();
    bool sizes = n == 6 && bulk[1].T.size() == n && per[0].T.size() == n && bulk[0].T.size() == n;
    CHECK("uvd_sequence_has_six_frames", sizes);
    if (!sizes) { cout << "FAILED" << endl; return fails; }
    bool same = true, poses = true, off_empty = true; int ran = 0, lines = 0; long moving_px = 0;
    for (size_t i = 0; i < n; i++) {
        const bool s = per[1].ran[i] == bulk[1].ran[i] && same_mat(per[1].moving[i], bulk[1].moving[i]) && same_mat(per[1].roi[i], bulk[1].roi[i]) && same_mat(per[1].ground[i], bulk[1].ground[i]) &&
                       memcmp(&per[1].pitch[i], &bulk[1].pitch[i], 8) == 0;
        if (!s) cout << "  frame " << i << ": ran " << per[1].ran[i] << " / " << bulk[1].ran[i] << " pitch " << per[1].pitch[i] << " / " << bulk[1].pitch[i] << " moving equal " << same_mat(per[1].moving[i], bulk[1].moving[i])
                     << " roi equal " << same_mat(per[1].roi[i], bulk[1].roi[i]) << " ground equal " << same_mat(per[1].ground[i], bulk[1].ground[i]) << endl;
        same = same && s;
        ran += per[1].ran[i]; lines += per[1].ran[i] && per[1].pitch[i] != 0.0;
        if (per[1].ran[i]) for (int r = 0; r < 120; r++) for (int c = 0; c < 400; c++) moving_px += per[1].moving[i].at<uchar>(r, c) == 255;
        for (const Run* r : {&per[1], &bulk[0], &bulk[1]}) poses = poses && memcmp(per[0].T[i].matrix().data(), r->T[i].matrix().data(), 128) == 0;
        off_empty = off_empty && per[0].moving[i].empty() && per[0].roi[i].empty() && per[0].ground[i].empty() && bulk[0].moving[i].empty() && bulk[0].roi[i].empty() && bulk[0].ground[i].empty();
    }
    cout << "  frames the stage ran on " << ran << ", with a ground line " << lines << ", moving pixels " << moving_px << endl;
    CHECK("uvd_tracker_and_bulk_tracker_give_the_same_masks_and_pitches", same);
    CHECK("uvd_stage_ran_and_found_a_ground_line", ran >= 4 && lines >= 3);
    CHECK("uvd_poses_do_not_depend_on_the_stage", poses);
    CHECK("uvd_off_leaves_the_masks_empty", off_empty);
    CHECK("uvd_some_frame_keeps_a_mask", moving_px > 0);
    // the redo path of BatchStereoTracker (argv[3]: the same scene with a jump of 150 px at image 4): with tracker_max_lost_frame = 0 the jump makes the tracker LOST,
    // the next frame goes through lostRecover, and from there to the end of the chunk the VO is redone per frame -- the inlier flags of those frames come from
    // ProcessMatches.  Chunks of 3 (the recovering frame inside a chunk), 4 (it opens one) and 8 (one chunk)
    if (argc > 3) {
        para.set("data_source", argv[3]); para.set("tracker_max_lost_frame", "0"); para.set("uv_disparity", "1");
        Run a; vector<int> Sa;
        {
            para.set("kitti_reader_depth", "1");
            Tracker tracker(para, vp); FrameReader rd(para, FrameReader::KITTI);
            while (RGBDFrame::Ptr f = rd.next()) {
                tracker.updateFrame(f);
                a.T.push_back(f->getTransform()); a.moving.push_back(f->moving_mask); a.roi.push_back(f->roi_mask); a.ground.push_back(f->ground_mask);
                a.ran.push_back(!f->moving_mask.empty()); a.pitch.push_back(f->moving_mask.empty() ? 0.0 : tracker.pitch1); Sa.push_back((int)tracker.getState());
            }
        }
        bool all = a.T.size() == 8; int lost = 0, redone = 0;
        for (int s : Sa) lost += s == Tracker::LOST;
        for (int chunk : {3, 4, 8}) {
            Run b; vector<int> Sb; int redo_ran = 0;
            para.set("kitti_reader_depth", "0");
            FrameReader rd(para, FrameReader::KITTI);
            BatchStereoTracker bs(para, vp, 400, 120, chunk);
            auto take = [&](const vector<RGBDFrame::Ptr>& done) {
                for (size_t i = 0; i < done.size(); i++) {
                    b.T.push_back(done[i]->getTransform()); b.moving.push_back(done[i]->moving_mask); b.roi.push_back(done[i]->roi_mask); b.ground.push_back(done[i]->ground_mask);
                    b.ran.push_back(bs.infos[i].uv); b.pitch.push_back(bs.infos[i].pitch1); Sb.push_back(bs.infos[i].state); redo_ran += bs.infos[i].uv && bs.infos[i].uv_redo;
                }
            };
            while (RGBDFrame::Ptr f = rd.next()) take(bs.push(f));
            take(bs.flush());
            para.set("kitti_reader_depth", "1");
            bool ok = b.T.size() == a.T.size();
            for (size_t i = 0; ok && i < a.T.size(); i++) {
                ok = a.ran[i] == b.ran[i] && Sa[i] == Sb[i] && same_mat(a.moving[i], b.moving[i]) && same_mat(a.roi[i], b.roi[i]) && same_mat(a.ground[i], b.ground[i]) && memcmp(&a.pitch[i], &b.pitch[i], 8) == 0 &&
                     memcmp(a.T[i].matrix().data(), b.T[i].matrix().data(), 128) == 0;
                if (!ok) cout << "  chunk " << chunk << " frame " << i << ": ran " << a.ran[i] << " / " << b.ran[i] << " state " << Sa[i] << " / " << Sb[i] << " pitch " << a.pitch[i] << " / " << b.pitch[i] << endl;
            }
            cout << "  chunk " << chunk << ": frames the stage ran on after a redone VO " << redo_ran << endl;
            all = all && ok; redone += redo_ran;
        }
        cout << "  lost frames " << lost << endl;
        CHECK("uvd_bulk_tracker_redo_path_equals_per_frame_tracker", all && lost >= 1 && redone >= 1);
    }
    cout << (fails ? "FAILED" : "ALL PASSED") << endl;
    return fails;
}
#endif
