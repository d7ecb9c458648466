// ctc_beam_demo.cpp -- CTC prefix beam search on the device through lele_amd/host/lele.hpp, end to end.
//   ctc_beam_demo probe        : builds and starts without a device
//   ctc_beam_demo run <dir>    : reads <dir>/{dims.i64 {k, skip_rows, blank, beam, nbest, width}, ids.i32 [R, k], lp.f32 [R, k], off.i64}.
//                                Writes <dir>/tokens.i32 [count, nbest, W], lengths.i32 and scores.f32 [count, nbest], counts.i32 [count]
//                                and shape.i64 {count, nbest, W} (ctc_beam_search_segments)
// Driven by tests/test_ctc_beam.py, which compares every file with the Python wrapper.
#include "lele.hpp"

#include <cstdio>
#include <cstring>
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
        std::printf("FAIL usage: ctc_beam_demo run <dir>\n");
        return 1;
    }
    try {
        namespace K = lele::kernels;
        const std::string d = std::string(argv[2]) + "/";
        const std::vector<int64_t> dims = read_file<int64_t>(d + "dims.i64"), off = read_file<int64_t>(d + "off.i64");
        const std::vector<int32_t> ids = read_file<int32_t>(d + "ids.i32");
        const std::vector<float> lp = read_file<float>(d + "lp.f32");
        if (dims.size() != 6 || off.empty() || dims[0] < 1) {
            std::printf("FAIL dims.i64 / off.i64\n");
            return 1;
        }
        const int64_t k = dims[0], rows = off.back();
        const TensorView ti = TensorView::from_slice(ids.data(), {rows, k}), tl = TensorView::from_slice(lp.data(), {rows, k});
        Buffer tok, len, sco, cnt;
        const auto hyp = K::ctc_beam_search_segments(ti, tl, off, dims[1], (int32_t)dims[2], (int32_t)dims[3], (int32_t)dims[4], dims[5], tok,
                                                     len, sco, cnt);
        write_file(d + "tokens.i32", hyp.tokens.to_vec<int32_t>());
        write_file(d + "lengths.i32", hyp.lengths.to_vec<int32_t>());
        write_file(d + "scores.f32", hyp.scores.to_vec<float>());
        write_file(d + "counts.i32", hyp.counts.to_vec<int32_t>());
        write_file(d + "shape.i64", hyp.tokens.shape);
        std::printf("OK rows=%lld segments=%lld beam=%d nbest=%d\n", (long long)rows, (long long)off.size() - 1, (int)dims[3], (int)dims[4]);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
