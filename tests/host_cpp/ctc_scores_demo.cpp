// ctc_scores_demo.cpp -- the scored greedy decode head of lele_amd/host/lele.hpp, end to end.
//   ctc_scores_demo probe        : builds and starts without a device
//   ctc_scores_demo run <dir>    : reads <dir>/{dims.i64 {K, N}, x.f32 [R, K], off.i64, w.f32 [K, N], ws.f32 [N], wz.f32 [1], b.f32 [N],
//                                  skip.u8 [V]}.  Writes <dir>/ids.i32 [R] and lp.f32 [R] (fused_quantized_linear_argmax_logprob_segments),
//                                  dense_ids.i32 [R] and dense_lp.f32 [R] (fused_quantized_linear_argmax_logprob on every segment alone),
//                                  kept.i32, frames.i32, kept_lp.f32 [count, W] and counts.i32 [count] (token_align_segments, width 0)
// Driven by tests/test_ctc_scores.py, which compares every file with the Python wrappers.
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
        std::printf("FAIL usage: ctc_scores_demo run <dir>\n");
        return 1;
    }
    try {
        namespace K = lele::kernels;
        const std::string d = std::string(argv[2]) + "/";
        const std::vector<int64_t> dims = read_file<int64_t>(d + "dims.i64"), off = read_file<int64_t>(d + "off.i64");
        const std::vector<float> x = read_file<float>(d + "x.f32"), w = read_file<float>(d + "w.f32"), ws = read_file<float>(d + "ws.f32"),
                                 wz = read_file<float>(d + "wz.f32"), b = read_file<float>(d + "b.f32");
        const std::vector<uint8_t> skip = read_file<uint8_t>(d + "skip.u8");
        if (dims.size() != 2 || off.empty()) {
            std::printf("FAIL dims.i64 / off.i64\n");
            return 1;
        }
        const int64_t k = dims[0], n = dims[1], rows = off.back(), count = (int64_t)off.size() - 1;
        const TensorView tx = TensorView::from_slice(x.data(), {rows, k});
        const TensorView tw = TensorView::weight(w.data(), {k, n}), tws = TensorView::from_slice(ws.data(), {n}),
                         twz = TensorView::from_slice(wz.data(), {1}), tb = TensorView::from_slice(b.data(), {n});
        const TensorView tskip = TensorView::from_slice(skip.data(), {(int64_t)skip.size()});
        Buffer ids_buf, lp_buf, one_ids, one_lp, kept_buf, frames_buf, kept_lp_buf, counts_buf;
        const auto head = K::fused_quantized_linear_argmax_logprob_segments(tx, off, tw, tws, twz, &tb, ids_buf, lp_buf);
        const std::vector<int32_t> ids_host = head.first.to_vec<int32_t>();
        const std::vector<float> lp_host = head.second.to_vec<float>();
        std::vector<int32_t> dense_ids;
        std::vector<float> dense_lp;
        for (int64_t i = 0; i < count; ++i) {
            const int64_t len = off[i + 1] - off[i];
            if (len == 0) continue;
            const TensorView seg = TensorView::from_slice(x.data() + off[i] * k, {len, k});
            const auto one = K::fused_quantized_linear_argmax_logprob(seg, tw, tws, twz, &tb, one_ids, one_lp);
            const std::vector<int32_t> a = one.first.to_vec<int32_t>();
            const std::vector<float> l = one.second.to_vec<float>();
            dense_ids.insert(dense_ids.end(), a.begin(), a.end());
            dense_lp.insert(dense_lp.end(), l.begin(), l.end());
        }
        const lele::kernels::AlignedTokens kept =
            K::token_align_segments(head.first, &head.second, off, tskip, 0, kept_buf, frames_buf, kept_lp_buf, counts_buf);
        write_file(d + "ids.i32", ids_host);
        write_file(d + "lp.f32", lp_host);
        write_file(d + "dense_ids.i32", dense_ids);
        write_file(d + "dense_lp.f32", dense_lp);
        write_file(d + "kept.i32", kept.ids.to_vec<int32_t>());
        write_file(d + "frames.i32", kept.frames.to_vec<int32_t>());
        write_file(d + "kept_lp.f32", kept.logprob.to_vec<float>());
        write_file(d + "counts.i32", kept.counts.to_vec<int32_t>());
        std::printf("OK rows=%lld segments=%lld\n", (long long)rows, (long long)count);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
