// The CPU side of tools/bench_kfgraph.py: the std::map restatement of kfgraph_restatement.h timed on the table the tool generated.  Reads the file
// the tool wrote (nine int64 counts, then the arrays in the order read below), builds the objects — one key point per observation, in ascending
// landmark order per key frame, so a candidate's items are its key points — and prints one JSON line: wall-clock milliseconds (median of `repeats`)
// of UpdateConnections for every key frame, of one UpdateLocalKeyFrames vote and of one culler pass over the candidates, with the sums the tool
// compares with the device's results.  usage: bench_kfgraph_ref FILE
#include <chrono>
#include <cstdint>
#include <cstdio>
#include "../../hyslam_amd/host/cv_compat.h"
#include "kfgraph_restatement.h"

template <class T> static std::vector<T> rd(FILE* f, int64_t n)
{
    std::vector<T> v((size_t)n);
    if (n > 0 && std::fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

template <class F> static double median_ms(int repeats, F f)
{
    std::vector<double> ms;
    for (int r = 0; r < repeats; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: bench_kfgraph_ref FILE\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int64_t> hd = rd<int64_t>(f, 9);
    const int64_t L = hd[0], n_kf = hd[1], n_obs = hd[2], n_local = hd[3], C = hd[4], n_items = hd[5], th = hd[6], th_obs = hd[7], repeats = hd[8];
    const auto off = rd<int64_t>(f, L + 1);
    const auto obs_kf = rd<int32_t>(f, n_obs), obs_oct = rd<int32_t>(f, n_obs);
    const auto lm_bad = rd<uint8_t>(f, L);
    const auto lm_nobs = rd<int32_t>(f, L);
    const auto kf_bad = rd<uint8_t>(f, n_kf);
    const auto kf_id = rd<int64_t>(f, n_kf);
    const auto local = rd<int32_t>(f, n_local);
    const auto cand_slot = rd<int32_t>(f, C);
    const auto cand_th = rd<float>(f, C);
    const auto cand_off = rd<int64_t>(f, C + 1);
    const auto item_depth = rd<float>(f, n_items);
    std::fclose(f);

    World W;
    std::vector<std::vector<cv::KeyPoint>> keys((size_t)n_kf);
    std::vector<std::vector<float>> depth((size_t)n_kf);
    for (int64_t o = 0; o < n_obs; o++) { cv::KeyPoint kp; kp.octave = obs_oct[o]; keys[obs_kf[o]].push_back(kp); depth[obs_kf[o]].push_back(1.0f); }
    for (int64_t c = 0; c < C; c++) {
        if ((int64_t)keys[cand_slot[c]].size() != cand_off[c + 1] - cand_off[c]) { std::fprintf(stderr, "candidate %lld: items are not its key points\n", (long long)c); return 2; }
        std::copy(item_depth.begin() + cand_off[c], item_depth.begin() + cand_off[c + 1], depth[cand_slot[c]].begin());
    }
    for (int64_t k = 0; k < n_kf; k++) {
        Camera cam; cam.sensor = 1;
        std::vector<FeatureDescriptor> d(keys[k].size());
        W.kfs.emplace_back(new KeyFrame(FeatureViews(keys[k], keys[k], std::vector<float>(keys[k].size(), -1.0f), depth[k], d, d, FeatureExtractorSettings()), cam));
        W.kfs.back()->mnId = (unsigned long)kf_id[k]; W.kfs.back()->mbBad = kf_bad[k] != 0;
    }
    std::vector<int> next((size_t)n_kf, 0);
    for (int64_t i = 0; i < L; i++) {
        W.lms.emplace_back(new MapPoint());
        MapPoint* lm = W.lms.back().get();
        lm->mbBad = lm_bad[i] != 0; lm->nObs = lm_nobs[i];
        for (int64_t o = off[i]; o < off[i + 1]; o++) {
            KeyFrame* p = W.kfs[obs_kf[o]].get();
            const int view = next[obs_kf[o]]++;
            p->associateLandMark(view, lm, true);
            lm->mObservations[p] = (size_t)view;
        }
    }
    for (int64_t c = 0; c < C; c++) { W.kfs[cand_slot[c]]->mThDepth = cand_th[c]; W.covisible.push_back(W.kfs[cand_slot[c]].get()); }

    long long sum_w = 0, sum_max = 0, sum_listed = 0;
    const double whole = median_ms((int)repeats, [&] {
        sum_w = sum_max = sum_listed = 0;
        for (int64_t k = 0; k < n_kf; k++) {
            std::map<KeyFrame*, int> counter; std::vector<KeyFrame*> ordered; std::vector<int> ws;
            ref_update_connections(W, W.kfs[k].get(), (int)th, counter, ordered, ws);
            int mx = 0;
            for (const auto& kc : counter) { sum_w += kc.second; mx = std::max(mx, kc.second); }
            sum_max += mx; sum_listed += (long long)ordered.size();
        }
    });
    std::vector<MapPoint*> matched;
    for (int32_t i : local) matched.push_back(W.lms[i].get());
    long long local_w = 0; int local_max = 0;
    const double votes = median_ms((int)repeats, [&] {
        std::map<KeyFrame*, int> counter; KeyFrame* kmax = nullptr;
        ref_local_votes(matched, counter, kmax, local_max);
        local_w = 0; for (const auto& kc : counter) local_w += kc.second;
    });
    Params prm; prm.LMobservations_thresh = (int)th_obs;
    long long sum_mps = 0, sum_red = 0, n_cull = 0;
    const double culler = median_ms((int)repeats, [&] {
        std::vector<int> snap; std::vector<std::pair<int, int>> counts;
        ref_cull(W, W.kfs[0].get(), prm, &snap, &counts);
        sum_mps = sum_red = 0; for (const auto& c : counts) { sum_mps += c.first; sum_red += c.second; }
        n_cull = (long long)snap.size();
    });
    std::printf("{\"whole_graph_ms\": %.4f, \"local_votes_ms\": %.4f, \"culler_ms\": %.4f, \"sum_weights\": %lld, \"sum_max_count\": %lld, \"sum_n_ordered\": %lld, "
                "\"local_sum_weights\": %lld, \"local_max_count\": %d, \"sum_n_mps\": %lld, \"sum_n_redundant\": %lld, \"n_cull\": %lld}\n",
                whole, votes, culler, sum_w, sum_max, sum_listed, local_w, local_max, sum_mps, sum_red, n_cull);
    return 0;
}
