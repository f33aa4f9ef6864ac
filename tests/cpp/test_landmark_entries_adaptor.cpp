// Exercises hyslam_amd/host/HipLandmarkEntries.h the way the hySLAM-side patch of INTEGRATION.md §9 uses it: per landmark its entry record, its
// observations and its descriptor set (host/cv_compat.h FeatureDescriptor) -> one call -> one Result per landmark.
// usage: test_landmark_entries_adaptor in.bin out.bin
//   in.bin   int32 L, hs_lm_entry_in[L], int64 obs_offsets[L+1], hs_lm_obs[obs_offsets[L]], int64 desc_offsets[L+1], uint8 desc[desc_offsets[L]][32]
//   out.bin  per landmark: float normal[3], min_dist, max_dist, mean_dist, size, int32 best, median, flags (rebuilt from the Result; unset
//            outputs written as 0) — from the calling thread's handle, then the same from an explicit handle (compared by the Python test)
// prints "LANDMARK ENTRIES ADAPTOR OK" on success, "NO DEVICE" without a GPU
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hyslam_amd/host/HipLandmarkEntries.h"

using namespace HYSLAM;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void put(FILE* o, const std::vector<HipLandmarkEntries::Result>& rs)
{
    for (const auto& r : rs) {
        float v[7] = {0, 0, 0, 0, 0, 0, r.size};
        if (r.normal_depth_set) {
            for (int c = 0; c < 3; c++) v[c] = r.normal.at<float>(c);
            v[3] = r.min_dist; v[4] = r.max_dist;
        }
        if (r.mean_set) v[5] = r.mean_dist;
        const int32_t flags = (r.normal_depth_set ? HS_LM_SET_NORMAL_DEPTH : 0) | (r.best >= 0 ? HS_LM_SET_DESC : 0) | (r.mean_set ? HS_LM_SET_MEAN : 0) |
                              HS_LM_SET_SIZE;
        const int32_t iv[3] = {r.best, r.median, flags};
        fwrite(v, 4, 7, o);
        fwrite(iv, 4, 3, o);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: test_landmark_entries_adaptor in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t L = 0;
    if (!rd(f, &L, 1) || L < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<hs_lm_entry_in> ent((size_t)L);
    std::vector<int64_t> ooff((size_t)L + 1), doff((size_t)L + 1);
    if (!rd(f, ent.data(), ent.size()) || !rd(f, ooff.data(), ooff.size())) { fprintf(stderr, "short read\n"); return 2; }
    std::vector<hs_lm_obs> obs((size_t)ooff[L]);
    if (!rd(f, obs.data(), obs.size()) || !rd(f, doff.data(), doff.size())) { fprintf(stderr, "short read\n"); return 2; }
    std::vector<uint8_t> desc((size_t)doff[L] * HS_DESC_BYTES);
    if (!rd(f, desc.data(), desc.size())) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    auto dist = std::make_shared<HipORBDistance>();
    std::vector<HipLandmarkEntries::Input> in((size_t)L);
    for (int32_t i = 0; i < L; i++) {
        in[i].entry = ent[i];
        in[i].observations.assign(obs.begin() + ooff[i], obs.begin() + ooff[i + 1]);
        for (int64_t j = doff[i]; j < doff[i + 1]; j++) {
            cv::Mat row(1, HS_DESC_BYTES, CV_8UC1);
            std::memcpy(row.ptr(0), desc.data() + j * HS_DESC_BYTES, HS_DESC_BYTES);
            in[i].descriptors.emplace_back(row, dist);
        }
    }

    int count = 0;
    if (hs_device_count(&count) != HS_OK || count < 1) { printf("NO DEVICE\n"); return 0; }
    std::vector<HipLandmarkEntries::Result> on_thread_r, explicit_r;
    try {
        HipLandmarkEntries on_thread;                                   // the calling thread's handle on the default device
        on_thread_r = on_thread.updateEntries(in);
        on_thread_r = on_thread.updateEntries(in);                      // a second call reuses the gather buffers and the handle's scratch
        hs_orb_params p; hs_orb_default_params(&p);
        hs_orb* h = nullptr;
        if (hs_orb_create(&p, 0, &h) != HS_OK) { printf("NO DEVICE\n"); return 0; }
        HipLandmarkEntries explicit_handle(h);
        explicit_r = explicit_handle.updateEntries(in);
        hs_orb_destroy(h);
    } catch (const std::exception& e) {
        printf("FAILED: %s\n", e.what());
        return 1;
    }
    if (on_thread_r.size() != (size_t)L || explicit_r.size() != (size_t)L) { printf("FAILED: result size\n"); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    put(o, on_thread_r);
    put(o, explicit_r);
    fclose(o);
    printf("LANDMARK ENTRIES ADAPTOR OK %d landmarks\n", (int)L);
    return 0;
}
