// Cross-check matching through the C++ layer (mim::Detector::set_filter, mim.hpp) on a planted binary
// dataset, which tests/test_cross_cpp.py writes as raw files.
//
// Every query set is a one-view model, every train set a scene scale.  detect_scene runs under
// MIM_FILTER_CROSS; the per-view n_good and status of last_results() are written for the test to compare
// with Python's match_batch(filter="cross") on the same sets.  The default filter must be MIM_FILTER_RATIO
// and give other records, and a filter outside 0..2 must throw mim::Error with MIM_EINVAL and change nothing.
//
// usage: cross_detector <dir> <n_models> <n_scenes> <nq> <nt> <width>   (dir holds q_<i>.u8, qkp_<i>.f32,
//        t_<j>.u8, tkp_<j>.f32; writes records.i32: n_good, status per view, model outer, scene inner)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "mim.hpp"

static std::vector<uint8_t> read_raw(const std::string& path, size_t n) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (v.size() != n) {
        std::fprintf(stderr, "bad size %zu for %s\n", v.size(), path.c_str());
        std::exit(2);
    }
    return v;
}

static std::vector<mim::Point2f> read_points(const std::string& path, size_t n) {
    const std::vector<uint8_t> raw = read_raw(path, n * sizeof(mim::Point2f));
    std::vector<mim::Point2f> p(n);
    if (n) std::memcpy(p.data(), raw.data(), raw.size());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: cross_detector <dir> <n_models> <n_scenes> <nq> <nt> <width>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int nm = std::atoi(argv[2]), ns = std::atoi(argv[3]), nq = std::atoi(argv[4]), nt = std::atoi(argv[5]),
              width = std::atoi(argv[6]);
    std::vector<mim::ModelViews> models(nm);
    std::vector<const mim::ModelViews*> mp;
    for (int i = 0; i < nm; ++i) {
        models[i].name = "model" + std::to_string(i);
        models[i].views.resize(1);
        mim::View& v = models[i].views[0];
        v.bin_descriptors = read_raw(dir + "/q_" + std::to_string(i) + ".u8", (size_t)nq * width);
        v.bin_width = width;
        v.keypoints = read_points(dir + "/qkp_" + std::to_string(i) + ".f32", nq);
        mp.push_back(&models[i]);
    }
    std::vector<std::vector<uint8_t>> tdesc(ns);
    std::vector<std::vector<mim::Point2f>> tkp(ns);
    std::vector<mim::Detector::ScaledScene> scales;
    for (int j = 0; j < ns; ++j) {
        tdesc[j] = read_raw(dir + "/t_" + std::to_string(j) + ".u8", (size_t)nt * width);
        tkp[j] = read_points(dir + "/tkp_" + std::to_string(j) + ".f32", nt);
    }
    for (int j = 0; j < ns; ++j) scales.push_back({&tkp[j], nullptr, 1.0f, &tdesc[j], width});
    try {
        mim::Detector det;
        if (det.filter() != MIM_FILTER_RATIO) {
            std::fprintf(stderr, "FAIL the default filter is %d\n", det.filter());
            return 1;
        }
        std::vector<std::vector<mim::Point2f>> out;
        det.detect_scene(mp, scales, out);
        const std::vector<mim_result> ratio = det.last_results();
        bool threw = false;
        try {
            det.set_filter(3);
        } catch (const mim::Error& e) {
            threw = e.status == MIM_EINVAL;
        }
        if (!threw || det.filter() != MIM_FILTER_RATIO) {
            std::fprintf(stderr, "FAIL set_filter(3) did not throw MIM_EINVAL\n");
            return 1;
        }
        det.set_filter(MIM_FILTER_CROSS);
        det.detect_scene(mp, scales, out);
        const std::vector<mim_result>& res = det.last_results();
        if (det.filter() != MIM_FILTER_CROSS || (int)res.size() != nm * ns || ratio.size() != res.size()) {
            std::fprintf(stderr, "FAIL %zu records under filter %d\n", res.size(), det.filter());
            return 1;
        }
        if (mim_last_kernel_ms(det.ctx(), "knn_cross") != 2.0) {
            std::fprintf(stderr, "FAIL knn_cross reads %g\n", mim_last_kernel_ms(det.ctx(), "knn_cross"));
            return 1;
        }
        std::vector<int32_t> rec;
        bool differs = false;
        size_t accepted = 0;
        for (size_t i = 0; i < res.size(); ++i) {
            rec.push_back(res[i].n_good);
            rec.push_back(res[i].status);
            differs |= res[i].n_good != ratio[i].n_good;
            accepted += res[i].status == MIM_ACCEPTED;
        }
        if (!differs) {
            std::fprintf(stderr, "FAIL the cross filter gave the ratio filter's good-match counts\n");
            return 1;
        }
        std::ofstream f(dir + "/records.i32", std::ios::binary);
        f.write(reinterpret_cast<const char*>(rec.data()), (std::streamsize)(rec.size() * sizeof(int32_t)));
        std::printf("OK cross detector: %d models x %d scenes, %zu accepted\n", nm, ns, accepted);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
