// Exercises hyslam_amd/host/HipLandmarkDescriptors.h the way the hySLAM-side patch of INTEGRATION.md §7 uses it: the observation descriptors of a
// batch of landmarks as std::vector<std::vector<FeatureDescriptor>> (host/cv_compat.h) -> one call -> the index of each landmark's representative.
// usage: test_landmark_adaptor in.bin out.bin
//   in.bin   int32 L, then per landmark int32 N and N x 32 descriptor bytes
//   out.bin  int32 best[L], int32 median[L] from the calling thread's handle, then the same from an explicit handle (compared by the Python test)
// prints "LANDMARK ADAPTOR OK" on success, "NO DEVICE" without a GPU
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hyslam_amd/host/HipLandmarkDescriptors.h"

using namespace HYSLAM;

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: test_landmark_adaptor in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t L = 0;
    if (fread(&L, 4, 1, f) != 1 || L < 0) { fprintf(stderr, "bad header\n"); return 2; }
    auto dist = std::make_shared<HipORBDistance>();
    std::vector<std::vector<FeatureDescriptor>> obs((size_t)L);
    for (int32_t i = 0; i < L; i++) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "bad landmark %d\n", i); return 2; }
        for (int32_t j = 0; j < n; j++) {
            cv::Mat row(1, HS_DESC_BYTES, CV_8UC1);
            if (fread(row.ptr(0), 1, HS_DESC_BYTES, f) != HS_DESC_BYTES) { fprintf(stderr, "short read\n"); return 2; }
            obs[i].emplace_back(row, dist);
        }
    }
    fclose(f);

    int count = 0;
    if (hs_device_count(&count) != HS_OK || count < 1) { printf("NO DEVICE\n"); return 0; }
    std::vector<int> med_thread, med_explicit;
    std::vector<int> best_thread, best_explicit;
    try {
        HipLandmarkDescriptors on_thread;                               // the calling thread's handle on the default device
        best_thread = on_thread.bestDescriptors(obs, &med_thread);
        best_thread = on_thread.bestDescriptors(obs, &med_thread);      // a second call reuses the gather buffers and the handle's scratch
        hs_orb_params p; hs_orb_default_params(&p);
        hs_orb* h = nullptr;
        if (hs_orb_create(&p, 0, &h) != HS_OK) { printf("NO DEVICE\n"); return 0; }
        HipLandmarkDescriptors explicit_handle(h);
        best_explicit = explicit_handle.bestDescriptors(obs, &med_explicit);
        hs_orb_destroy(h);
    } catch (const std::exception& e) {
        printf("FAILED: %s\n", e.what());
        return 1;
    }
    if (best_thread.size() != (size_t)L || med_thread.size() != (size_t)L) { printf("FAILED: result size\n"); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const std::vector<int>* outs[4] = {&best_thread, &med_thread, &best_explicit, &med_explicit};
    for (const std::vector<int>* v : outs)
        for (int x : *v) { const int32_t y = x; fwrite(&y, 4, 1, o); }
    fclose(o);
    printf("LANDMARK ADAPTOR OK %d landmarks\n", (int)L);
    return 0;
}
