// ssm/uvdisparity.hpp -- UVDisparity (reference include/uvdisparity.hpp, include/basicStructure.hpp, src/uvdisparity.cpp): the moving-object detector of the
// stereo path, same public surface: the parameter setters and Process() with the reference's signature.  Process() is ssm_uvd_process of libssm_hip.so when
// the calling thread has a device context (the one its OrbFeature used last, as for Looper), otherwise ssm_uvd_process_host; both run the arithmetic of
// include/ssm/uvd_core.h and give the same bits.  It edits vo.quadmatches_inlier / vo.quadmatches_outlier the way filterInOut does.  The
// 10-channel xyz image of triangulate10D is never materialised: the parameter is kept and left untouched.  Set the parameters before the first Process():
// the two Kalman filters live in the library object, which is created then.
#pragma once
#include "common_headers.h"
#include "device.h"
#include "orb.h"
#include "vo_stereo.hpp"

struct ROI3D {                      // basicStructure.hpp:15-38
    ROI3D() : x_max(30000), y_max(-1000), z_max(30000) {}
    ROI3D(double x, double y, double z) { x_max = x; y_max = y; z_max = z; }
    double x_max, y_max, z_max;
};
struct CalibPars {                  // basicStructure.hpp:42-95
    CalibPars() : f(0.0), c_x(0.0), c_y(0.0), b(0.0) {}
    CalibPars(const double _f, const double _cx, const double _cy, const double _base) { f = _f; c_x = _cx; c_y = _cy; b = _base; }
    double f, c_x, c_y, b;
};
struct USegmentPars {               // uvdisparity.hpp:17-36
    USegmentPars() : min_intense(32), min_disparity_raw(64), min_area(40) {}
    USegmentPars(int min_intense_, int min_disparity_raw_, int min_area_) { min_intense = min_intense_; min_disparity_raw = min_disparity_raw_; min_area = min_area_; }
    int min_intense, min_disparity_raw, min_area;
};

class UVDisparity {
public:
    UVDisparity() { out_th_ = 6.0f; inlier_tolerance_ = 3; min_adjust_intense_ = 19; }
    ~UVDisparity() { if (uvd_) ssm_uvd_destroy(uvd_); }
    UVDisparity(const UVDisparity&) = delete; UVDisparity& operator=(const UVDisparity&) = delete;
    inline void SetCalibPars(CalibPars& calib_par) { calib_ = calib_par; }
    inline void SetROI3D(ROI3D& roi_3d) { roi_ = roi_3d; }
    inline void SetUSegmentPars(int min_intense, int min_disparity_raw, int min_area) {
        this->u_segment_par_.min_intense = min_intense; this->u_segment_par_.min_disparity_raw = min_disparity_raw; this->u_segment_par_.min_area = min_area;
    }
    inline void SetOutThreshold(double out_th) { out_th_ = out_th; }                               // (set and never read in the reference either)
    inline void SetInlierTolerance(int inlier_tolerance) { inlier_tolerance_ = inlier_tolerance; }
    inline void SetMinAdjustIntense(int min_adjust_intense) { min_adjust_intense_ = min_adjust_intense; }   // (likewise)
    // -> the moving mask (CV_8UC1, 255 = moving); roi_mask / ground_mask (CV_8UC1) and the measured pitch are filled; xyz is left as it is
    cv::Mat Process(cv::Mat& img_L, cv::Mat& disp_sgbm, VisualOdometryStereo& vo, cv::Mat& xyz, cv::Mat& roi_mask, cv::Mat& ground_mask, double& pitch1, double& pitch2) {
        if (img_L.empty() || img_L.type() != CV_8UC1 || disp_sgbm.type() != CV_16SC1 || disp_sgbm.rows != img_L.rows || disp_sgbm.cols != img_L.cols || disp_sgbm.step != 2 * img_L.step)
            throw std::invalid_argument("UVDisparity::Process: an 8-bit left image and its CV_16SC1 disparity with the same element stride");
        ensure();
        const int w = img_L.cols, h = img_L.rows;
        // the VO's two lists as one array with inlier flags, inliers first: each list keeps its order
        std::vector<ssm_pmatch> m; std::vector<uint8_t> fl;
        static_assert(sizeof(pmatch) == sizeof(ssm_pmatch), "pmatch layout");
        for (const pmatch& q : vo.quadmatches_inlier) { ssm_pmatch t; memcpy(&t, &q, sizeof t); m.push_back(t); fl.push_back(1); }
        for (const pmatch& q : vo.quadmatches_outlier) { ssm_pmatch t; memcpy(&t, &q, sizeof t); m.push_back(t); fl.push_back(0); }
        cv::Mat mask_moving(h, w, CV_8UC1);
        roi_mask.create(h, w, CV_8UC1); ground_mask.create(h, w, CV_8UC1);
        const int rc = (dev_ ? ssm_uvd_process : ssm_uvd_process_host)(uvd_, img_L.data, disp_sgbm.ptr<int16_t>(), w, h, (int)img_L.step, m.data(), fl.data(), (int)m.size(),
                                                                      mask_moving.data, roi_mask.data, ground_mask.data, &last_info);
        if (rc != SSM_OK) throw ssm::DeviceError(rc, std::string("ssm_uvd_process: ") + (dev_ ? ssm_last_error(dev_->ctx()) : "bad arguments"));
        vo.quadmatches_inlier.clear(); vo.quadmatches_outlier.clear();
        for (size_t i = 0; i < m.size(); i++) {
            if (fl[i] & 2) continue;                                    // erased by filterInOut
            pmatch q; memcpy(static_cast<void*>(&q), &m[i], sizeof q);
            (fl[i] & 1 ? vo.quadmatches_inlier : vo.quadmatches_outlier).push_back(q);
        }
        pitch1 = last_info.pitch_measured; pitch2 = last_info.pitch_measured;       // line2 is fitted to pt_list too (uvdisparity.cpp:437-438)
        return mask_moving;
    }
    bool onDevice() const { return dev_ != nullptr; }
    ssm_uvd_info last_info{};           // of the most recent Process (not in the reference's class)
private:
    void ensure() {
        if (uvd_) return;
        ssm_uvd_params p; ssm_uvd_params_default(&p);
        p.f = calib_.f; p.cu = calib_.c_x; p.cv = calib_.c_y; p.base = calib_.b;
        p.roi_x = roi_.x_max; p.roi_y = roi_.y_max; p.roi_z = roi_.z_max;
        p.min_intense = u_segment_par_.min_intense; p.min_disparity_raw = u_segment_par_.min_disparity_raw; p.min_area = u_segment_par_.min_area;
        p.inlier_tolerance = inlier_tolerance_;
        dev_ = rgbd_tutor::OrbFeature::lastDevice();
        const int rc = ssm_uvd_create(dev_ ? dev_->ctx() : nullptr, &p, &uvd_);
        if (rc != SSM_OK) throw ssm::DeviceError(rc, std::string("ssm_uvd_create: ") + ssm_last_error(dev_ ? dev_->ctx() : nullptr));
    }
    CalibPars calib_; ROI3D roi_; USegmentPars u_segment_par_;
    double out_th_; int inlier_tolerance_, min_adjust_intense_;
    ssm_uvd* uvd_ = nullptr; ssm::Device* dev_ = nullptr;
};
