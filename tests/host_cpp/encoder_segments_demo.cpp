// encoder_segments_demo.cpp -- the four packed-batch wrappers of lele_amd/host/lele.hpp (segments_prepend, fused_quantized_linear_segments,
// depthwise_conv1d_tlc_segments, attention_segments), end to end.
//   encoder_segments_demo probe        : builds and starts without a device
//   encoder_segments_demo run <dir>    : reads <dir>/{qkv.f32 [R, 1536], off.i64, fsmn.f32 [512, 1, 11], w.f32 [512, 512], ws.f32 [512],
//                                        b.f32 [512], prefix.f32 [4, 1536]}; writes <dir>/{pre.f32, preoff.i64, mem.f32, att.f32, lin.f32}
// Driven by tests/test_encoder_segments.py, which compares every file with the Python wrappers bit for bit.
#include "lele.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

using lele::Buffer;
using lele::TensorView;

template <typename T>
static std::vector<T> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(b.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}
template <typename T>
static void write_file(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "probe";
    if (mode == "probe") {
        std::printf("PROBE\n");
        return 0;
    }
    if (mode != "run" || argc < 3) {
        std::printf("FAIL usage: encoder_segments_demo run <dir>\n");
        return 1;
    }
    try {
        namespace K = lele::kernels;
        const std::string d = std::string(argv[2]) + "/";
        const std::vector<float> qkv = read_file<float>(d + "qkv.f32"), fsmn = read_file<float>(d + "fsmn.f32"), w = read_file<float>(d + "w.f32"),
                                 ws = read_file<float>(d + "ws.f32"), b = read_file<float>(d + "b.f32"), prefix = read_file<float>(d + "prefix.f32");
        const std::vector<int64_t> off = read_file<int64_t>(d + "off.i64");
        const float zero = 128.0f, scale = 0.08838834764831845f;  // 128^-0.5
        const int64_t rows = off.back();
        Buffer o_pre, o_mem, o_att, o_lin;
        std::vector<int64_t> preoff;
        const TensorView x = TensorView::from_slice(qkv.data(), {rows, 1536});
        const TensorView pre = K::segments_prepend(x, off, TensorView::from_slice(prefix.data(), {4, 1536}), o_pre, preoff);
        const TensorView mem = K::depthwise_conv1d_tlc_segments(pre, preoff, TensorView::weight(fsmn.data(), {512, 1, 11}), nullptr, 5, 5, false,
                                                                1024, true, o_mem);
        const TensorView sc = TensorView::from_slice(&scale, {1});
        const TensorView att = K::attention_segments(pre, preoff, 0, 512, 1024, 4, 128, &sc, o_att);
        const TensorView bias = TensorView::weight(b.data(), {512});
        const TensorView lin = K::fused_quantized_linear_segments(att, preoff, TensorView::weight(w.data(), {512, 512}), TensorView::weight(ws.data(), {512}),
                                                                  TensorView::from_slice(&zero, {1}), &bias, false, o_lin);
        write_file(d + "pre.f32", pre.to_vec<float>());
        write_file(d + "preoff.i64", preoff);
        write_file(d + "mem.f32", mem.to_vec<float>());
        write_file(d + "att.f32", att.to_vec<float>());
        write_file(d + "lin.f32", lin.to_vec<float>());
        std::printf("OK rows=%lld segments=%zu\n", (long long)preoff.back(), off.size() - 1);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
