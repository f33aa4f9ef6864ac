// Exercises hyslam_amd/host/HipPlaceRecognizer.h through its plain-data core (keys, std::map BoW vectors, covisibility lists), the way the
// KeyFrame* overloads of INTEGRATION.md §10 use it.
// usage: test_place_adaptor in.bin out.bin
//   in.bin   int32 n_words, n_kf; per key frame: uint64 key, int32 m, int32 word[m], double value[m], int32 n_nb, uint64 nb[n_nb];
//            int32 n_erased, uint64 erased[]; int32 n_queries; per query: int32 loop, float min_score, int32 m, word[m], value[m], int32 n_conn, uint64 conn[]
//   out.bin  per query: int32 n, uint64 key[n]
// prints "PLACE ADAPTOR OK" on success, "NO DEVICE" without a GPU
#include <cstdio>
#include <cstdlib>
#include <map>
#include "../../hyslam_amd/host/HipPlaceRecognizer.h"

using namespace HYSLAM;

template <class T> static T rd(FILE* f) { T v{}; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short read\n"); exit(2); } return v; }

static std::map<unsigned, double> rd_bow(FILE* f)
{
    const int32_t m = rd<int32_t>(f);
    std::vector<int32_t> w((size_t)m);
    std::map<unsigned, double> bow;
    for (auto& x : w) x = rd<int32_t>(f);
    for (int32_t i = 0; i < m; i++) bow[(unsigned)w[i]] = rd<double>(f);
    return bow;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: test_place_adaptor in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int count = 0;
    if (hs_device_count(&count) != HS_OK || count < 1) { printf("NO DEVICE\n"); return 0; }
    try {
        const int32_t n_words = rd<int32_t>(f), n_kf = rd<int32_t>(f);
        HipPlaceRecognizer rec(n_words);                              // the calling thread's handle
        std::map<uint64_t, std::vector<uint64_t>> nbs;
        for (int32_t i = 0; i < n_kf; i++) {
            const uint64_t key = rd<uint64_t>(f);
            rec.add(key, rd_bow(f));
            const int32_t n_nb = rd<int32_t>(f);
            for (int32_t j = 0; j < n_nb; j++) nbs[key].push_back(rd<uint64_t>(f));
        }
        const int32_t n_erased = rd<int32_t>(f);
        for (int32_t i = 0; i < n_erased; i++) rec.erase(rd<uint64_t>(f));
        if (rec.size() != (size_t)(n_kf - n_erased)) { printf("FAILED: size\n"); return 1; }
        const HipPlaceRecognizer::Neighbours neighbours = [&nbs](uint64_t k) { return nbs[k]; };
        FILE* o = fopen(argv[2], "wb");
        if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        const int32_t n_queries = rd<int32_t>(f);
        for (int32_t q = 0; q < n_queries; q++) {
            const int32_t loop = rd<int32_t>(f);
            const float min_score = rd<float>(f);
            const std::map<unsigned, double> bow = rd_bow(f);
            std::set<uint64_t> conn;
            const int32_t n_conn = rd<int32_t>(f);
            for (int32_t j = 0; j < n_conn; j++) conn.insert(rd<uint64_t>(f));
            const std::vector<uint64_t> out = loop ? rec.detectLoopCandidates(bow, conn, min_score, neighbours) : rec.detectRelocalizationCandidates(bow, neighbours);
            const int32_t n = (int32_t)out.size();
            fwrite(&n, 4, 1, o);
            fwrite(out.data(), 8, out.size(), o);
        }
        fclose(o);
        rec.clear();
        if (rec.size() != 0) { printf("FAILED: clear\n"); return 1; }
        printf("PLACE ADAPTOR OK %d key frames, %d queries\n", (int)n_kf, (int)n_queries);
    } catch (const std::exception& e) {
        printf("FAILED: %s\n", e.what());
        return 1;
    }
    fclose(f);
    return 0;
}
