// test_png_write.cpp -- ssm::imwritePNG (include/ssm/png_io.h) against ssm::imreadPNG: what is written reads back as the same Mat, for 8-bit gray, 8-bit BGR and
// 16-bit gray images of several sizes (widths 1 and 67 among them), from packed and from strided Mats; what the writer does not take is refused.  Host only, no
// device call, no library: runs in the CPU test suite, also under the sanitizers.
#include "ssm/png_io.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unistd.h>
#include <vector>
using namespace std;

static int failures = 0;
static void check(bool ok, const string& name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str()); if (!ok) failures++; }
struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };

static bool same(const cv::Mat& a, const cv::Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || a.type() != b.type()) return false;
    for (int y = 0; y < a.rows; y++) if (memcmp(a.ptr<uint8_t>(y), b.ptr<uint8_t>(y), (size_t)a.cols * a.elemSize())) return false;
    return true;
}
static cv::Mat random_mat(int w, int h, int type, Rng& r, int kind)
{
    cv::Mat m(h, w, type);
    for (int y = 0; y < h; y++) {
        uint8_t* p = m.ptr<uint8_t>(y);
        for (size_t i = 0; i < (size_t)w * m.elemSize(); i++) p[i] = kind == 0 ? (uint8_t)r.next() : kind == 1 ? 0 : (uint8_t)(y + i / 7);          // noise, flat, smooth
    }
    return m;
}

int main()
{
    const char* dir = getenv("TMPDIR");
    const string path = string(dir && *dir ? dir : "/tmp") + "/ssm_test_png_write_" + to_string((long)getpid()) + ".png";
    Rng r{12345};
    const int sizes[][2] = {{1, 1}, {1, 9}, {67, 5}, {9, 7}, {64, 3}, {640, 48}, {1241, 3}};
    const int types[] = {CV_8UC1, CV_8UC3, CV_16UC1};
    const char* names[] = {"8UC1", "8UC3", "16UC1"};
    for (auto& sz : sizes) for (int t = 0; t < 3; t++) for (int kind = 0; kind < 3; kind++) {
        const cv::Mat m = random_mat(sz[0], sz[1], types[t], r, kind);
        const bool ok = ssm::imwritePNG(path, m);
        const cv::Mat back = ssm::imreadPNG(path, -1);
        check(ok && same(m, back), string("round trip ") + names[t] + " " + to_string(sz[0]) + "x" + to_string(sz[1]) + " kind " + to_string(kind));
    }
    {   // a 16-bit image with every byte order trap: 0x00FF, 0xFF00, 0x0100, 0xFFFF
        cv::Mat m(1, 4, CV_16UC1);
        const uint16_t v[4] = {0x00FF, 0xFF00, 0x0100, 0xFFFF};
        memcpy(m.ptr<uint16_t>(0), v, 8);
        check(ssm::imwritePNG(path, m) && same(m, ssm::imreadPNG(path, -1)), "16-bit byte order");
    }
    {   // BGR in, BGR out: the default flag reads the colours back in the same order
        cv::Mat m(1, 2, CV_8UC3);
        const uint8_t v[6] = {1, 2, 3, 250, 128, 0};
        memcpy(m.ptr<uint8_t>(0), v, 6);
        check(ssm::imwritePNG(path, m) && same(m, ssm::imreadPNG(path)), "BGR order");
    }
    {   // a strided Mat: rows of a wider buffer
        vector<uint8_t> buf(10 * 40, 7);
        for (size_t i = 0; i < buf.size(); i++) buf[i] = (uint8_t)(i * 13);
        cv::Mat m(10, 11, CV_8UC3, buf.data(), 40);
        check(ssm::imwritePNG(path, m) && same(m.clone(), ssm::imreadPNG(path, -1)), "strided rows");
    }
    check(!ssm::imwritePNG(path, cv::Mat()), "an empty Mat is refused");
    check(!ssm::imwritePNG(path, cv::Mat(2, 2, CV_32FC1)), "a float Mat is refused");
    check(!ssm::imwritePNG("/nonexistent-directory/x.png", cv::Mat(2, 2, CV_8UC1)), "an unwritable path is refused");
    remove(path.c_str());
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
