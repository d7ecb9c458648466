// rnn_segments_demo.cpp -- lstm_segments / gru_segments of lele_amd/host/lele.hpp, end to end.
//   rnn_segments_demo probe        : builds and starts without a device
//   rnn_segments_demo run <dir>    : reads <dir>/{dims.i64 {I, H}, x.f32 [R, I], off.i64, w.f32 [1, 4H, I], r.f32 [1, 4H, H], b.f32 [8H],
//                                    h0.f32 [count, H], c0.f32 [count, H]}; the GRU takes the first 3H rows of w / r and the halves
//                                    [0, 3H) and [4H, 7H) of b.  Writes <dir>/{ly, lh, lc, gy, gh}.f32 and info.i32 {lstm form, NS, gru form, NS}
// Driven by tests/test_rnn_segments.py, which compares every file with the Python wrappers bit for bit.
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
        std::printf("FAIL usage: rnn_segments_demo run <dir>\n");
        return 1;
    }
    try {
        namespace K = lele::kernels;
        const std::string d = std::string(argv[2]) + "/";
        const std::vector<int64_t> dims = read_file<int64_t>(d + "dims.i64"), off = read_file<int64_t>(d + "off.i64");
        const std::vector<float> x = read_file<float>(d + "x.f32"), w = read_file<float>(d + "w.f32"), r = read_file<float>(d + "r.f32"),
                                 b = read_file<float>(d + "b.f32"), h0 = read_file<float>(d + "h0.f32"), c0 = read_file<float>(d + "c0.f32");
        if (dims.size() != 2 || off.empty()) {
            std::printf("FAIL dims.i64 / off.i64\n");
            return 1;
        }
        const int64_t in = dims[0], h = dims[1], rows = off.back(), count = (int64_t)off.size() - 1;
        std::vector<float> b3(b.begin(), b.begin() + 3 * h);
        b3.insert(b3.end(), b.begin() + 4 * h, b.begin() + 7 * h);
        const TensorView tx = TensorView::from_slice(x.data(), {rows, in});
        const TensorView th = TensorView::from_slice(h0.data(), {1, count, h}), tc = TensorView::from_slice(c0.data(), {1, count, h});
        const TensorView tb = TensorView::from_slice(b.data(), {8 * h}), tb3 = TensorView::from_slice(b3.data(), {6 * h});
        Buffer ly, lh, lc, gy, gh;
        std::vector<int32_t> info(4, -1);
        const K::LstmOut lo = K::lstm_segments(tx, off, TensorView::weight(w.data(), {1, 4 * h, in}), TensorView::weight(r.data(), {1, 4 * h, h}),
                                               &tb, &th, &tc, ly, lh, lc, info.data());
        const K::GruOut go = K::gru_segments(tx, off, TensorView::from_slice(w.data(), {1, 3 * h, in}), TensorView::from_slice(r.data(), {1, 3 * h, h}),
                                             &tb3, &th, false, gy, gh, info.data() + 2);
        write_file(d + "ly.f32", lo.y.to_vec<float>());
        write_file(d + "lh.f32", lo.h.to_vec<float>());
        write_file(d + "lc.f32", lo.c.to_vec<float>());
        write_file(d + "gy.f32", go.y.to_vec<float>());
        write_file(d + "gh.f32", go.h.to_vec<float>());
        write_file(d + "info.i32", info);
        std::printf("OK rows=%lld segments=%lld\n", (long long)rows, (long long)count);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
