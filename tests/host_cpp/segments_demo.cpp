// segments_demo.cpp -- SenseVoiceFrontend::compute_segments + Cmvn::compute_segments of lele_amd/host/lele.hpp, end to end.
//   segments_demo probe                                  : builds and starts without a device
//   segments_demo run <pcm.f32> <segs.i64> <feats.f32> <cmvn.f32> <offsets.i64>
//       segs: (start, end) pairs; writes the packed features, their per-segment CMVN and the row offsets
// Driven by tests/test_frontend_segments.py, which compares each segment with the Python compute().
#include "lele.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <utility>
#include <vector>

using lele::Buffer;
using lele::TensorView;

template <typename T>
static std::vector<T> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(b.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}
template <typename T>
static void write_file(const char* path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "probe";
    if (mode == "probe") {
        std::printf("PROBE\n");
        return 0;
    }
    if (mode != "run" || argc < 7) {
        std::printf("FAIL usage: segments_demo run <pcm.f32> <segs.i64> <feats.f32> <cmvn.f32> <offsets.i64>\n");
        return 1;
    }
    try {
        const std::vector<float> pcm = read_file<float>(argv[2]);
        const std::vector<int64_t> raw = read_file<int64_t>(argv[3]);
        std::vector<std::pair<int64_t, int64_t>> segs;
        for (size_t i = 0; i + 1 < raw.size(); i += 2) segs.emplace_back(raw[i], raw[i + 1]);
        lele::features::SenseVoiceFrontend fe;
        Buffer o_feat, o_cmvn;
        std::vector<int64_t> offsets;
        TensorView feats = fe.compute_segments(TensorView::from_slice(pcm.data(), {(int64_t)pcm.size()}), segs, o_feat, offsets);
        TensorView norm = lele::features::Cmvn().compute_segments(feats, offsets, o_cmvn);
        write_file(argv[4], feats.to_vec<float>());
        write_file(argv[5], norm.to_vec<float>());
        write_file(argv[6], offsets);
        std::printf("OK rows=%lld segments=%zu\n", (long long)offsets.back(), segs.size());
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
