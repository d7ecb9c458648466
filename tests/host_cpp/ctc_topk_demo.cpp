// ctc_topk_demo.cpp -- the k-best decode head of lele_amd/host/lele.hpp, end to end.
//   ctc_topk_demo probe        : builds and starts without a device
//   ctc_topk_demo run <dir>    : reads <dir>/{dims.i64 {K, N, k}, x.f32 [R, K], off.i64, w.f32 [K, N], ws.f32 [N], wz.f32 [1], b.f32 [N]}.
//                                Writes <dir>/ids.i32 [R, k] and lp.f32 [R, k] (fused_quantized_linear_topk_segments), dense_ids.i32 and
//                                dense_lp.f32 [R, k] (fused_quantized_linear_topk on every segment alone)
// Driven by tests/test_ctc_topk.py, which compares every file with the Python wrappers.
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
        std::printf("FAIL usage: ctc_topk_demo run <dir>\n");
        return 1;
    }
    try {
        namespace K = lele::kernels;
        const std::string d = std::string(argv[2]) + "/";
        const std::vector<int64_t> dims = read_file<int64_t>(d + "dims.i64"), off = read_file<int64_t>(d + "off.i64");
        const std::vector<float> x = read_file<float>(d + "x.f32"), w = read_file<float>(d + "w.f32"), ws = read_file<float>(d + "ws.f32"),
                                 wz = read_file<float>(d + "wz.f32"), b = read_file<float>(d + "b.f32");
        if (dims.size() != 3 || off.empty()) {
            std::printf("FAIL dims.i64 / off.i64\n");
            return 1;
        }
        const int64_t k = dims[0], n = dims[1], rows = off.back(), count = (int64_t)off.size() - 1;
        const int32_t best = (int32_t)dims[2];
        const TensorView tx = TensorView::from_slice(x.data(), {rows, k});
        const TensorView tw = TensorView::weight(w.data(), {k, n}), tws = TensorView::from_slice(ws.data(), {n}),
                         twz = TensorView::from_slice(wz.data(), {1}), tb = TensorView::from_slice(b.data(), {n});
        Buffer ids_buf, lp_buf, one_ids, one_lp;
        const auto head = K::fused_quantized_linear_topk_segments(tx, off, tw, tws, twz, &tb, best, ids_buf, lp_buf);
        std::vector<int32_t> dense_ids;
        std::vector<float> dense_lp;
        for (int64_t i = 0; i < count; ++i) {
            const int64_t len = off[i + 1] - off[i];
            if (len == 0) continue;
            const TensorView seg = TensorView::from_slice(x.data() + off[i] * k, {len, k});
            const auto one = K::fused_quantized_linear_topk(seg, tw, tws, twz, &tb, best, one_ids, one_lp);
            const std::vector<int32_t> a = one.first.to_vec<int32_t>();
            const std::vector<float> l = one.second.to_vec<float>();
            dense_ids.insert(dense_ids.end(), a.begin(), a.end());
            dense_lp.insert(dense_lp.end(), l.begin(), l.end());
        }
        write_file(d + "ids.i32", head.first.to_vec<int32_t>());
        write_file(d + "lp.f32", head.second.to_vec<float>());
        write_file(d + "dense_ids.i32", dense_ids);
        write_file(d + "dense_lp.f32", dense_lp);
        std::printf("OK rows=%lld segments=%lld k=%d\n", (long long)rows, (long long)count, (int)best);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
