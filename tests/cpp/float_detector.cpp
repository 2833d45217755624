// Generic float descriptors through the C++ layer (mim::View::float_dim, Detector::ScaledScene::float_dim,
// mim.hpp) on the planted float dataset, which tests/test_float_cpp.py writes as raw files.
//
// Every query set is a one-view model, every train set a scene scale.  The per-model points of
// detect_scene are written for the test to compare with Python's batch_inlier_points on the same sets.
// The same call again must reuse the registered views and give the same points.  A generic float model
// against a 128-D scene, and against a scene of another float_dim, must throw mim::Error with MIM_EINVAL
// and leave the Detector usable.
//
// usage: float_detector <dir> <dim> <n_models> <n_scenes> <nq>... <nt>... <scale>...   (dir holds q_<i>.f32,
//        qkp_<i>.f32, t_<j>.f32, tkp_<j>.f32; writes pts_<i>.f32)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "mim.hpp"

static std::vector<float> read_floats(const std::string& path, size_t n) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() != n * sizeof(float)) {
        std::fprintf(stderr, "bad size %zu for %s\n", raw.size(), path.c_str());
        std::exit(2);
    }
    std::vector<float> v(n);
    if (n) std::memcpy(v.data(), raw.data(), raw.size());
    return v;
}

static std::vector<mim::Point2f> read_points(const std::string& path, size_t n) {
    const std::vector<float> raw = read_floats(path, 2 * n);
    std::vector<mim::Point2f> p(n);
    if (n) std::memcpy(p.data(), raw.data(), sizeof(mim::Point2f) * n);
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
    if (argc < 5) {
        std::fprintf(stderr, "usage: float_detector <dir> <dim> <n_models> <n_scenes> <nq>... <nt>... <scale>...\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int dim = std::atoi(argv[2]), nm = std::atoi(argv[3]), ns = std::atoi(argv[4]);
    if (argc != 5 + nm + 2 * ns) {
        std::fprintf(stderr, "%d arguments for %d models and %d scenes\n", argc - 5, nm, ns);
        return 2;
    }
    std::vector<mim::ModelViews> models(nm);
    std::vector<const mim::ModelViews*> mp;
    for (int i = 0; i < nm; ++i) {
        const int nq = std::atoi(argv[5 + i]);
        models[i].name = "model" + std::to_string(i);
        models[i].views.resize(1);
        mim::View& v = models[i].views[0];
        v.descriptors = read_floats(dir + "/q_" + std::to_string(i) + ".f32", (size_t)nq * dim);
        v.float_dim = dim;
        v.keypoints = read_points(dir + "/qkp_" + std::to_string(i) + ".f32", nq);
        mp.push_back(&models[i]);
    }
    std::vector<std::vector<float>> tdesc(ns);
    std::vector<std::vector<mim::Point2f>> tkp(ns);
    std::vector<mim::Detector::ScaledScene> scales;
    for (int j = 0; j < ns; ++j) {
        const int nt = std::atoi(argv[5 + nm + j]);
        tdesc[j] = read_floats(dir + "/t_" + std::to_string(j) + ".f32", (size_t)nt * dim);
        tkp[j] = read_points(dir + "/tkp_" + std::to_string(j) + ".f32", nt);
    }
    for (int j = 0; j < ns; ++j)
        scales.push_back({&tkp[j], &tdesc[j], (float)std::atof(argv[5 + nm + ns + j]), nullptr, 0, dim});
    try {
        mim::Detector det;
        std::vector<std::vector<mim::Point2f>> out, again;
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
        if (nm < 2 || out[0].empty() || out[1].empty() || same(out[0], out[1])) {
            std::fprintf(stderr, "FAIL models 0 and 1 must have distinct, non-empty points\n");
            return 1;
        }
        // a generic float model against a 128-D scene, then against a scene of another float_dim
        std::vector<float> other(tkp[0].size() * 128, 0.f);
        int threw = 0;
        for (int k = 0; k < 2; ++k) {
            try {
                std::vector<std::vector<mim::Point2f>> none;
                if (k == 0)
                    det.detect_scene(mp, {{&tkp[0], &other, 1.0f}}, none);
                else
                    det.detect_scene(mp, {{&tkp[0], &other, 1.0f, nullptr, 0, dim == 128 ? 64 : 128}}, none);
            } catch (const mim::Error& e) {
                threw += e.status == MIM_EINVAL;
                std::printf("mixed kinds: %s\n", e.what());
            }
        }
        if (threw != 2) {
            std::fprintf(stderr, "FAIL a kind or dim mismatch did not throw MIM_EINVAL (%d of 2)\n", threw);
            return 1;
        }
        // the Detector is still usable, and the registered views are reused: the same points again
        det.detect_scene(mp, scales, again);
        for (int i = 0; i < nm; ++i)
            if (!same(out[i], again[i])) {
                std::fprintf(stderr, "FAIL second call: model %d differs\n", i);
                return 1;
            }
        std::printf("OK float detector: dim %d, %d models x %d scenes, %zu points\n", dim, nm, ns, total);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAIL exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
