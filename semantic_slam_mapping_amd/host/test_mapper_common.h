// test_mapper_common.h -- what the programs that drive a Mapper on the device share (test_motion_fuse, test_sor, test_carve, test_render, test_align, test_grid,
// test_relabel): the PASS / FAIL lines, a Mapper whose viewer thread has ended, and the byte comparisons.  Each program is one translation unit, so `fails` is its own.
#pragma once
#include "ssm/rgbdframe.h"
#include "ssm/track.h"
#include "ssm/pose_graph.h"
#include "ssm/mapper.h"
#include "ssm/vo_stereo.hpp"
using namespace std;
using namespace rgbd_tutor;
static int fails = 0;
#define CHECK(name, cond) do { if (cond) cout << "PASS " << name << endl; else { cout << "FAIL " << name << endl; fails++; } } while (0)

// a Mapper whose viewer thread has ended, so that its device and its two routes can be driven from here
struct QuietMapper : Mapper {
    QuietMapper(const ParameterReader& p, PoseGraph& g) : Mapper(p, g) { shutdown(); }
    ~QuietMapper() { for (auto& kv : devClouds) ssm_cloud_free(dev ? dev->ctx() : nullptr, kv.second); devClouds.clear(); }
    vector<ssm_point> deviceRoute(const RGBDFrame::Ptr& f, const double* T = nullptr) {          // the device cloud as it is now: camera frame, or transformed by T
        ssm_cloud* cl = deviceCloud(f);
        ssm::Device& d = device(f->depth.cols, f->depth.rows);
        vector<ssm_point> out((size_t)max(ssm_cloud_size(cl), 1)); int n = 0;
        d.check(ssm_cloud_fetch(d.ctx(), cl, T, out.data(), (int)out.size(), &n), "ssm_cloud_fetch");
        out.resize((size_t)n);
        return out;
    }
    vector<ssm_point> hostRoute(const RGBDFrame::Ptr& f) {                                        // frame->pointcloud as it is now
        hostCloud(f);
        return points(*f->pointcloud);
    }
    vector<ssm_point> cloudNow(const RGBDFrame::Ptr& f) { return device_map ? deviceRoute(f) : hostRoute(f); }      // by the mapper's own route
    // the two routes to a key-frame's world-frame cloud, made afresh: the device cloud is dropped again
    vector<ssm_point> viaDevice(const RGBDFrame::Ptr& f) {
        const Eigen::Isometry3d T = f->getTransform();
        vector<ssm_point> out = deviceRoute(f, T.data());
        ssm_cloud_free(device(f->depth.cols, f->depth.rows).ctx(), devClouds[f.get()]); devClouds.erase(f.get());
        return out;
    }
    vector<ssm_point> viaHost(const RGBDFrame::Ptr& f) { return points(*generatePointCloud(f)); }
    const vector<uint8_t>* runOf(const RGBDFrame::Ptr& f) const { auto it = carveRun.find(f.get()); return it == carveRun.end() ? nullptr : &it->second; }
    // view j once more, and what ssm_render_fetch gives for it
    void fetchView(const vector<RGBDFrame::Ptr>& kfs, size_t j, cv::Mat& dep, cv::Mat& bgr, cv::Mat& lab) {
        RenderTarget t;
        renderView(kfs, j, t);
        dep.create(t.h, t.w, CV_16UC1); bgr.create(t.h, t.w, CV_8UC3); lab.create(t.h, t.w, CV_8UC1);
        ssm::Device& d = device(t.w, t.h);
        d.check(ssm_render_fetch(d.ctx(), t.t, dep.ptr<uint16_t>(), bgr.data, lab.data, nullptr), "ssm_render_fetch");
    }
    ssm::Device& dev_(int w, int h) { return device(w, h); }
    static vector<ssm_point> points(const PointCloud& c) {
        vector<ssm_point> out(c.points.size());
        if (!out.empty()) memcpy((void*)out.data(), c.points.data(), out.size() * sizeof(ssm_point));
        return out;
    }
};
static inline bool same(const vector<ssm_point>& a, const vector<ssm_point>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (memcmp(&a[i], &b[i], 16) != 0 || a[i].b != b[i].b || a[i].g != b[i].g || a[i].r != b[i].r || a[i].label != b[i].label) return false;
    return true;
}
static inline bool same_pose(const Eigen::Isometry3d& a, const Eigen::Isometry3d& b) { return memcmp(a.data(), b.data(), 16 * sizeof(double)) == 0; }
static inline bool same_mat(const cv::Mat& a, const cv::Mat& b)
{
    if (a.empty() || a.rows != b.rows || a.cols != b.cols || a.type() != b.type()) return false;
    for (int y = 0; y < a.rows; y++) if (memcmp(a.ptr<uint8_t>(y), b.ptr<uint8_t>(y), (size_t)a.cols * a.elemSize())) return false;
    return true;
}
