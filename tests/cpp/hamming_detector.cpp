// Binary descriptors through the C++ layer (mim::View::bin_descriptors, Detector::detect_scene, mim.hpp) on
// the planted binary dataset, which tests/test_hamming_cpp.py writes as raw files.
//
// Every query set is a one-view model, every train set a scene scale.  The per-model points of
// detect_scene are written for the test to compare with Python's batch_inlier_points on the same sets.
// Then model 0's view is rewritten in place with model 1's rows and keypoints: after invalidate_models the
// next call must give model 0 the points model 1 had.  A binary model against a float scene must throw
// mim::Error with MIM_EINVAL and leave the Detector usable.
//
// usage: hamming_detector <dir> <n_models> <n_scenes> <nq> <nt> <width> <scale>...   (dir holds q_<i>.u8,
//        qkp_<i>.f32, t_<j>.u8, tkp_<j>.f32; writes pts_<i>.f32 and, after the rewrite, pts2_<i>.f32)
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

static void write_points(const std::string& path, const std::vector<mim::Point2f>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(mim::Point2f)));
}

static bool same(const std::vector<mim::Point2f>& a, const std::vector<mim::Point2f>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(mim::Point2f) * a.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: hamming_detector <dir> <n_models> <n_scenes> <nq> <nt> <width> <scale>...\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int nm = std::atoi(argv[2]), ns = std::atoi(argv[3]), nq = std::atoi(argv[4]), nt = std::atoi(argv[5]),
              width = std::atoi(argv[6]);
    if (argc != 7 + ns) {
        std::fprintf(stderr, "%d scales for %d scenes\n", argc - 7, ns);
        return 2;
    }
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
    for (int j = 0; j < ns; ++j) scales.push_back({&tkp[j], nullptr, (float)std::atof(argv[7 + j]), &tdesc[j], width});
    try {
        mim::Detector det;
        std::vector<std::vector<mim::Point2f>> out, again, out2;
        det.detect_scene(mp, scales, out);
        if ((int)out.size() != nm || (int)det.last_results().size() != nm * ns) {
            std::fprintf(stderr, "FAIL %zu models out, %zu records\n", out.size(), det.last_results().size());
            return 1;
        }
        size_t total = 0;
        for (int i = 0; i < nm; ++i) {
            write_points(dir + "/pts_" + std::to_string(i) + ".f32", out[i]);
            total += out[i].size();
        }
        // the registered views are reused: the same call again gives the same points
        det.detect_scene(mp, scales, again);
        for (int i = 0; i < nm; ++i)
            if (!same(out[i], again[i])) {
                std::fprintf(stderr, "FAIL second call: model %d differs\n", i);
                return 1;
            }
        if (nm < 2 || out[0].empty() || out[1].empty() || same(out[0], out[1])) {
            std::fprintf(stderr, "FAIL models 0 and 1 must have distinct, non-empty points (%zu, %zu)\n",
                         nm > 0 ? out[0].size() : 0, nm > 1 ? out[1].size() : 0);
            return 1;
        }
        // a binary model against a float scene: the library's MIM_EINVAL as mim::Error
        std::vector<float> fdesc((size_t)nt * 128, 0.f);
        bool threw = false;
        try {
            std::vector<std::vector<mim::Point2f>> none;
            det.detect_scene(mp, {{&tkp[0], &fdesc, 1.0f}}, none);
        } catch (const mim::Error& e) {
            threw = e.status == MIM_EINVAL;
            std::printf("mixed kinds: %s\n", e.what());
        }
        if (!threw) {
            std::fprintf(stderr, "FAIL a binary model against a float scene did not throw MIM_EINVAL\n");
            return 1;
        }
        // model 0's view rewritten in place (same storage) with model 1's rows and keypoints
        std::memcpy(models[0].views[0].bin_descriptors.data(), models[1].views[0].bin_descriptors.data(), (size_t)nq * width);
        std::memcpy(models[0].views[0].keypoints.data(), models[1].views[0].keypoints.data(), sizeof(mim::Point2f) * nq);
        det.invalidate_models();
        det.detect_scene(mp, scales, out2);
        for (int i = 0; i < nm; ++i) write_points(dir + "/pts2_" + std::to_string(i) + ".f32", out2[i]);
        if (!same(out2[0], out[1]) || !same(out2[1], out[1])) {
            std::fprintf(stderr, "FAIL the rewritten view was not seen (%zu points, model 1 has %zu)\n", out2[0].size(),
                         out[1].size());
            return 1;
        }
        std::printf("OK hamming detector: %d models x %d scenes, %zu points\n", nm, ns, total);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
