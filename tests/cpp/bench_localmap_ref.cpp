// The CPU side of tools/bench_local_map.py: the host assembly of the local map — the literal restatement of localmap_restatement.h — timed on the
// table the tool generated.  Reads the file the tool wrote (eight int64 counts, then the arrays in the order read below), builds the objects and
// prints one JSON line: wall-clock milliseconds (median of `repeats`) of UpdateLocalKeyFrames + UpdateLocalPoints + the filter of SearchLocalPoints,
// with the counts the tool compares with the device's results.  usage: bench_localmap_ref FILE
#include <chrono>
#include <cstdint>
#include <cstdio>
#include "../../hyslam_amd/host/cv_compat.h"
#include "localmap_restatement.h"

template <class T> static std::vector<T> rd(FILE* f, int64_t n)
{
    std::vector<T> v((size_t)n);
    if (n > 0 && std::fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: bench_localmap_ref FILE\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int64_t> hd = rd<int64_t>(f, 8);
    const int64_t L = hd[0], n_kf = hd[1], n_obs = hd[2], n_assoc = hd[3], neigh_cap = hd[4], repeats = hd[5];
    TrackLocalMapParameters params;
    params.N_max_local_keyframes = (int)hd[6]; params.N_neighbor_keyframes = (int)hd[7];
    const auto off = rd<int64_t>(f, L + 1);
    const auto obs_kf = rd<int32_t>(f, n_obs);
    const auto lm_bad = rd<uint8_t>(f, L);
    const auto kf_bad = rd<uint8_t>(f, n_kf);
    const auto neigh = rd<int32_t>(f, n_kf * neigh_cap), parent = rd<int32_t>(f, n_kf), frame_lm = rd<int32_t>(f, n_assoc);
    std::fclose(f);

    MapWorld W;
    std::vector<size_t> n_views((size_t)n_kf, 0);
    for (int64_t o = 0; o < n_obs; o++) n_views[obs_kf[o]]++;
    for (int64_t k = 0; k < n_kf; k++) {
        Camera cam; cam.sensor = 1;
        const std::vector<cv::KeyPoint> keys(n_views[k]);
        const std::vector<FeatureDescriptor> d(n_views[k]);
        const std::vector<float> none(n_views[k], -1.0f);
        W.kfs.emplace_back(new KeyFrame(FeatureViews(keys, keys, none, none, d, d, FeatureExtractorSettings()), cam));
        W.kfs.back()->mnId = (unsigned long)k; W.kfs.back()->mbBad = kf_bad[k] != 0;
    }
    std::vector<int> next((size_t)n_kf, 0);
    std::map<MapPoint*, int64_t> index;
    for (int64_t i = 0; i < L; i++) {
        W.lms.emplace_back(new MapPoint());
        MapPoint* lm = W.lms.back().get();
        index[lm] = i;
        lm->mbBad = lm_bad[i] != 0;
        for (int64_t o = off[i]; o < off[i + 1]; o++) {
            KeyFrame* p = W.kfs[obs_kf[o]].get();
            const int view = next[obs_kf[o]]++;
            p->associateLandMark(view, lm, true);
            lm->mObservations[p] = (size_t)view; lm->nObs++;
        }
    }
    for (int64_t k = 0; k < n_kf; k++) {
        for (int64_t j = 0; j < neigh_cap; j++) if (neigh[k * neigh_cap + j] >= 0) W.ordered[W.kfs[k].get()].push_back(W.kfs[neigh[k * neigh_cap + j]].get());
        if (parent[k] >= 0) W.kfs[k]->mpParent = W.kfs[parent[k]].get();
    }
    Frame F;
    for (int64_t a = 0; a < n_assoc; a++) if (frame_lm[a] >= 0) F.associateLandMark((int)a, W.lms[frame_lm[a]].get(), true);

    Literal out;
    std::vector<double> ms;
    for (int r = 0; r < (int)repeats + 1; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        out = literal(F, &W, params);
        if (r > 0) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    long long sum_sel = 0;
    for (MapPoint* p : out.v_lmp) sum_sel += index[p];
    std::printf("{\"assembly_ms\": %.4f, \"assembly_min_ms\": %.4f, \"n_local\": %zu, \"n_sel\": %zu, \"sum_sel\": %lld, \"n_removed\": %zu}\n",
                ms[ms.size() / 2], ms[0], out.local_key_frames.size(), out.v_lmp.size(), sum_sel, out.removed.size());
    return 0;
}
