// Scene images in, inlier points out, over a group of devices (mim::GroupDetector, mim.hpp; the C entries
// mim_group_scene_images_run / mim_group_scene_points) on the reference's sugar_box images, which
// tests/test_group_images.py writes as raw files: processAllTestImages' scene loop (Output.cpp:23-57).
//
// The model is built with Detector::sift per view; the baseline is Detector::detect_scene_gray per scene
// on one ctx.  Groups over {0}, {0,0}, {0,0,0} and, with two or more GPUs, {0,1} and every device run a
// batch of all the scenes, of two scenes (over 3 ranks one rank has none), of none, and of the colour
// copies (B = G = R = gray, which the conversion maps back to the same gray).  Every scene's points and
// records must be the baseline's byte for byte.  The 3-rank group's points and boxes are written for
// the test to compare with the golden outputs.
//
// usage: group_images <dir> <rows> <cols> <n_views> <scene>...   (dir holds view_<i>.u8, mask_<i>.u8,
//        scene_<name>.u8, scene_<name>.bgr; writes pts_<name>.f32 and boxes_<name>.i32)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "mim.hpp"
#include "mim_detect.hpp"

static std::vector<uint8_t> read_raw(const std::string& path, size_t n) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (v.size() != n) {
        std::fprintf(stderr, "bad size %zu for %s\n", v.size(), path.c_str());
        std::exit(2);
    }
    return v;
}

template <class T>
static void write_raw(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::fprintf(stderr, "FAIL "); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");    \
            return false;                  \
        }                                  \
    } while (0)

using ScenePts = std::vector<std::vector<mim::Point2f>>;  // per model

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One batch through the group: points and records against the baseline's first scenes.size() scenes,
// and the capacity convention of mim_group_scene_points.
static bool run_batch(mim::GroupDetector& gd, const char* what, const std::vector<mim_image>& scenes,
                      const std::vector<float>& scales, const std::vector<ScenePts>& base_pts,
                      const std::vector<std::vector<mim_result>>& base_res, std::vector<ScenePts>* keep = nullptr) {
    std::vector<ScenePts> out;
    gd.detect_scenes(scenes, scales, out);
    const size_t nt = gd.templates_per_scene();
    CHECK(out.size() == scenes.size(), "%s: %zu scenes out for %zu in", what, out.size(), scenes.size());
    CHECK(gd.last_results().size() == scenes.size() * nt, "%s: %zu records", what, gd.last_results().size());
    for (size_t i = 0; i < scenes.size(); ++i) {
        CHECK(nt == base_res[i].size(), "%s: %zu templates, baseline has %zu records", what, nt, base_res[i].size());
        CHECK(std::memcmp(&gd.last_results()[i * nt], base_res[i].data(), sizeof(mim_result) * nt) == 0,
              "%s: scene %zu: records differ from the baseline's", what, i);
        CHECK(out[i].size() == base_pts[i].size(), "%s: scene %zu: %zu models", what, i, out[i].size());
        for (size_t m = 0; m < out[i].size(); ++m) {
            CHECK(out[i][m].size() == base_pts[i][m].size(), "%s: scene %zu model %zu: %zu points, baseline %zu", what, i,
                  m, out[i][m].size(), base_pts[i][m].size());
            CHECK(out[i][m].empty() || std::memcmp(out[i][m].data(), base_pts[i][m].data(),
                                                   sizeof(mim::Point2f) * out[i][m].size()) == 0,
                  "%s: scene %zu model %zu: points differ from the baseline's", what, i, m);
        }
        // a buffer one point short: MIM_ERANGE, the offsets still those of the full call
        std::vector<int64_t> offs(nt + 1, -1), offs2(nt + 1, -2);
        CHECK(mim_group_scene_points(gd.group(), (int32_t)i, nullptr, 0, offs.data()) == MIM_OK, "%s: offsets only", what);
        if (offs[nt] > 0) {
            std::vector<float> buf((size_t)offs[nt] * 2);
            const mim_status s = mim_group_scene_points(gd.group(), (int32_t)i, buf.data(), offs[nt] - 1, offs2.data());
            CHECK(s == MIM_ERANGE, "%s: scene %zu: cap one short gave status %d", what, i, s);
            CHECK(offs == offs2, "%s: scene %zu: offsets differ after MIM_ERANGE", what, i);
        }
    }
    if (keep) *keep = out;
    return true;
}

// A batch that fails after it has begun (its second scene has two channels, which the rank's image
// entry refuses) leaves no batch: records and points are errors with a text, until a batch succeeds.
// After a descriptor-set batch the points are MIM_EINVAL (the group does not know its scales).
static bool failure_state(mim::GroupDetector& gd, const char* what, const std::vector<mim_image>& scenes,
                          const std::vector<float>& scales, const std::vector<ScenePts>& base_pts,
                          const std::vector<std::vector<mim_result>>& base_res) {
    std::vector<mim_image> bad(scenes.begin(), scenes.begin() + 2);
    bad[1].channels = 2;
    bad[1].cols /= 2;
    std::vector<ScenePts> out;
    bool threw = false;
    try {
        gd.detect_scenes(bad, scales, out);
    } catch (const mim::Error& e) {
        threw = e.status == MIM_EINVAL && std::strstr(e.what(), "channels") != nullptr;
    }
    CHECK(threw, "%s: a two-channel scene did not fail with MIM_EINVAL and a text", what);
    std::vector<mim_result> rec(2 * gd.templates_per_scene());
    std::vector<int64_t> offs(gd.templates_per_scene() + 1);
    CHECK(mim_group_results(gd.group(), rec.data()) != MIM_OK, "%s: records after a failed batch", what);
    CHECK(std::strlen(mim_group_last_error(gd.group())) > 0, "%s: no text after a failed batch", what);
    CHECK(mim_group_scene_points(gd.group(), 0, nullptr, 0, offs.data()) != MIM_OK, "%s: points after a failed batch", what);
    CHECK(std::strlen(mim_group_last_error(gd.group())) > 0, "%s: no text after a failed batch", what);
    const std::vector<mim_image> two(scenes.begin(), scenes.begin() + 2);
    if (!run_batch(gd, "two scenes after a failed batch", two, scales, base_pts, base_res)) return false;
    mim_params prm;
    mim_default_params(&prm);
    CHECK(mim_group_scene_batch_run(gd.group(), 0, 1, nullptr, 0, nullptr, &prm) == MIM_OK, "%s: empty set batch", what);
    CHECK(mim_group_results(gd.group(), nullptr) == MIM_OK, "%s: empty set batch results", what);
    CHECK(mim_group_scene_points(gd.group(), 0, nullptr, 0, offs.data()) == MIM_EINVAL,
          "%s: points after a descriptor-set batch", what);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const std::string dir = argv[1];
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), nv = std::atoi(argv[4]);
    const size_t px = (size_t)rows * cols;
    const std::vector<float> scales = {0.7f, 0.85f, 1.0f, 1.15f, 1.3f};  // TestsDetector.cpp:99
    std::vector<std::string> names(argv + 5, argv + argc);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        std::fprintf(stderr, "FAIL no HIP device\n");
        return 1;
    }
    std::printf("devices visible: %d\n", ndev);
    try {
        mim::Detector det(0);
        mim::ModelViews model;
        model.name = "004_sugar_box";
        for (int i = 0; i < nv; ++i) {
            const auto gray = read_raw(dir + "/view_" + std::to_string(i) + ".u8", px);
            const auto mask = read_raw(dir + "/mask_" + std::to_string(i) + ".u8", px);
            std::vector<mim_keypoint> kps;
            mim::View v;
            det.sift(gray.data(), rows, cols, cols, mask.data(), cols, kps, v.descriptors);
            for (const auto& k : kps) v.keypoints.push_back({k.x, k.y});
            model.views.push_back(std::move(v));
        }
        std::vector<std::vector<uint8_t>> gray, bgr;
        std::vector<mim_image> gimg, cimg;
        for (const auto& n : names) {
            gray.push_back(read_raw(dir + "/scene_" + n + ".u8", px));
            bgr.push_back(read_raw(dir + "/scene_" + n + ".bgr", px * 3));
        }
        for (size_t i = 0; i < names.size(); ++i) {
            gimg.push_back(mim_image{gray[i].data(), rows, cols, 1, cols});
            cimg.push_back(mim_image{bgr[i].data(), rows, cols, 3, (int64_t)cols * 3});
        }
        // baseline: one ctx, scene by scene
        std::vector<ScenePts> base_pts(names.size());
        std::vector<std::vector<mim_result>> base_res(names.size());
        for (size_t i = 0; i < names.size(); ++i) {
            det.detect_scene_gray({&model}, gray[i].data(), rows, cols, cols, scales, base_pts[i]);
            base_res[i] = det.last_results();
        }
        {  // detect_scene_image: gray is detect_scene_gray, colour converts first
            ScenePts p;
            det.detect_scene_image({&model}, cimg[0], scales, p);
            if (p[0].size() != base_pts[0][0].size() ||
                std::memcmp(p[0].data(), base_pts[0][0].data(), sizeof(mim::Point2f) * p[0].size()) != 0 ||
                std::memcmp(det.last_results().data(), base_res[0].data(), sizeof(mim_result) * base_res[0].size()) != 0) {
                std::fprintf(stderr, "FAIL detect_scene_image(colour) differs from detect_scene_gray\n");
                return 1;
            }
        }
        std::vector<std::vector<int>> lists = {{0}, {0, 0}, {0, 0, 0}};
        if (ndev >= 2) {
            lists.push_back({0, 1});
            std::vector<int> all;
            for (int d = 0; d < ndev; ++d) all.push_back(d);
            if (ndev > 2) lists.push_back(all);
        }
        const std::vector<mim_image> two(gimg.begin(), gimg.begin() + std::min<size_t>(2, gimg.size()));
        for (const auto& devs : lists) {
            std::string label;
            for (int d : devs) label += (label.empty() ? "{" : ",") + std::to_string(d);
            label += "}";
            bool distinct = true;
            for (size_t a = 0; a < devs.size(); ++a)
                for (size_t b = a + 1; b < devs.size(); ++b) distinct &= devs[a] != devs[b];
            mim::GroupDetector gd(devs);
            gd.set_models({&model});
            if (mim_group_uses_rccl(gd.group()) != (distinct ? 1 : 0)) {
                std::fprintf(stderr, "FAIL group %s: uses_rccl %d\n", label.c_str(), mim_group_uses_rccl(gd.group()));
                return 1;
            }
            std::vector<ScenePts> kept;
            if (!run_batch(gd, (label + " all scenes").c_str(), gimg, scales, base_pts, base_res, &kept)) return 1;
            if (devs.size() == 1) {
                // scenes/s of the group of one and of the Detector loop: both warm, five passes each,
                // alternating; every pass ends with its points on the host
                std::vector<double> tg, td;
                std::vector<ScenePts> out;
                ScenePts p;
                for (int rep = 0; rep < 5; ++rep) {
                    double t0 = now_s();
                    for (size_t i = 0; i < names.size(); ++i)
                        det.detect_scene_gray({&model}, gray[i].data(), rows, cols, cols, scales, p);
                    td.push_back(names.size() / (now_s() - t0));
                    t0 = now_s();
                    gd.detect_scenes(gimg, scales, out);
                    tg.push_back(names.size() / (now_s() - t0));
                }
                std::sort(tg.begin(), tg.end());
                std::sort(td.begin(), td.end());
                std::printf("scenes/s, %zu scenes, median (min-max) of 5: GroupDetector{0} %.0f (%.0f-%.0f), Detector loop "
                            "%.0f (%.0f-%.0f)\n", names.size(), tg[2], tg[0], tg[4], td[2], td[0], td[4]);
            }
            if (!run_batch(gd, (label + " two scenes").c_str(), two, scales, base_pts, base_res)) return 1;
            if (!run_batch(gd, (label + " no scene").c_str(), {}, scales, base_pts, base_res)) return 1;
            if (!run_batch(gd, (label + " colour scenes").c_str(), cimg, scales, base_pts, base_res)) return 1;
            if (!failure_state(gd, label.c_str(), gimg, scales, base_pts, base_res)) return 1;
            std::printf("group %s (rccl %d): OK\n", label.c_str(), mim_group_uses_rccl(gd.group()));
            if (devs.size() == 3 && !distinct) {
                for (size_t i = 0; i < names.size(); ++i) {
                    std::vector<float> flat;
                    for (const auto& p : kept[i][0]) {
                        flat.push_back(p.x);
                        flat.push_back(p.y);
                    }
                    write_raw(dir + "/pts_" + names[i] + ".f32", flat);
                    mim::Detections dets;
                    mim::boxes_for_model(kept[i][0], model.name, dets);
                    std::vector<int32_t> boxes;
                    for (const auto& d : dets) {
                        boxes.push_back(d.first.x);
                        boxes.push_back(d.first.y);
                        boxes.push_back(d.first.width);
                        boxes.push_back(d.first.height);
                    }
                    write_raw(dir + "/boxes_" + names[i] + ".i32", boxes);
                }
            }
        }
        if (ndev >= 2) std::printf("distinct-device groups ran\n");
        else std::printf("SKIP distinct-device: %d GPU\n", ndev);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL %s\n", e.what());
        return 1;
    }
    std::printf("OK group images\n");
    return 0;
}
