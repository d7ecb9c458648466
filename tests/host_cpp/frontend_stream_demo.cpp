// frontend_stream_demo.cpp -- lele::features::FrontendStream of lele_amd/host/lele.hpp: one live stream pushed chunk by chunk.
//   frontend_stream_demo probe                                  : builds and starts without a device
//   frontend_stream_demo rows <samples_before> <chunk_len> <final>
//       the closed forms of one push on the default config (host arithmetic): rows, new frames, samples and log-mel rows carried
//   frontend_stream_demo run <pcm.f32> <cuts.i64> <feats.f32> <counts.i64>
//       cuts: k + 1 sample positions; chunk j = pcm[cuts[j], cuts[j + 1]), the last one final.  Writes the rows of every push one after
//       another and how many each push returned.
// Driven by tests/test_frontend_stream.py, which compares the rows with the Python FrontendStream and with compute() on the whole pcm.
#include "lele.hpp"

#include <cstdio>
#include <cstdlib>
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
    try {
        if (mode == "rows" && argc >= 5) {
            const lele::features::StreamRows r =
                lele::features::stream_rows(lele::features::FeatureConfig(), std::atoll(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]) != 0);
            std::printf("ROWS %lld %lld %lld %lld\n", (long long)r.rows, (long long)r.new_frames, (long long)r.pcm_carry, (long long)r.mel_carry);
            return 0;
        }
        if (mode != "run" || argc < 6) {
            std::printf("FAIL usage: frontend_stream_demo run <pcm.f32> <cuts.i64> <feats.f32> <counts.i64>\n");
            return 1;
        }
        const std::vector<float> pcm = read_file<float>(argv[2]);
        const std::vector<int64_t> cuts = read_file<int64_t>(argv[3]);
        int64_t max_chunk = 1;
        for (size_t j = 0; j + 1 < cuts.size(); ++j) max_chunk = std::max(max_chunk, cuts[j + 1] - cuts[j]);
        lele::features::SenseVoiceFrontend fe;
        lele::features::FrontendStream stream(fe, 1, max_chunk);
        const TensorView all = TensorView::from_slice(pcm.data(), {(int64_t)pcm.size()});
        Buffer out;
        std::vector<float> feats;
        std::vector<int64_t> counts, offsets;
        for (size_t j = 0; j + 1 < cuts.size(); ++j) {
            const bool last = j + 2 == cuts.size();
            TensorView rows = stream.push(all, {{cuts[j], cuts[j + 1]}}, {(uint8_t)last}, out, offsets);
            counts.push_back(offsets.back());
            if (offsets.back()) {
                const std::vector<float> v = rows.to_vec<float>();
                feats.insert(feats.end(), v.begin(), v.end());
            }
        }
        const lele::features::FrontendStream::Counters c = stream.counters(0);
        if (c.samples != 0 || c.frames != 0 || c.rows != 0) {
            std::printf("FAIL the final push left the stream at %lld samples\n", (long long)c.samples);
            return 1;
        }
        write_file(argv[4], feats);
        write_file(argv[5], counts);
        std::printf("OK pushes=%zu rows=%zu\n", counts.size(), feats.size() / 560);
        return 0;
    } catch (const lele::Error& e) {
        std::printf("FAIL lele::Error: %s\n", e.what());
        return 1;
    }
}
