// adaptor_threads.cpp — the thread code of the header-only adaptors (hyslam_amd/host/) under a sanitizer, CPU only: built against the library's
// host-only objects and hip_stub.cpp instead of libhyslam_amd.so (tests/cpp/host_sanitize/Makefile; ThreadSanitizer with SAN=thread, AddressSanitizer +
// UndefinedBehaviorSanitizer otherwise).  No kernel runs under the stub, so no match is checked here (tests/test_adaptor.py holds the searches to the
// oracle on the GPU); what runs for real is what the adaptors do with threads:
//   hip_detail::Worker         run / wait, many jobs on one helper, an exception in a job (wait() rethrows, the helper lives on), a Worker that
//                              never ran, destruction with a job outstanding
//   hip_detail::thread_handle  one handle per calling thread, the same one again on the same thread, destroyed when its thread exits while the
//                              other threads go on working on theirs
//   HipFeatureMatcher          SearchByProjection over 5000 cv_compat landmarks (from 4096 on the gather splits the landmarks BY FIELD: helpers
//                              fill the geometry, the caller the descriptors), from two calling threads at once, each with helpers of its own;
//                              HYSLAM_AMD_GATHER_THREADS = 0, 1, 2 is read once per process: the test runs this program once per value
// usage: adaptor_threads        prints "ADAPTOR THREADS OK ..."
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <set>
#include <stdexcept>
#include <thread>
#include <vector>
#include <dirent.h>
#include "../../../hyslam_amd/host/HipORBFactory.h"

using namespace HYSLAM;
extern "C" void hip_stub_zero_device();

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Gate {
    std::atomic<int> waiting{0}; const int n;
    explicit Gate(int n_) : n(n_) {}
    void arrive() { waiting++; while (waiting.load() < n) std::this_thread::yield(); }
};

static int worker_section()
{
    {
        hip_detail::Worker idle;                                 // never ran: no thread to join
    }
    hip_detail::Worker w;
    long sum = 0;                                                // written by the helper, read by the caller after wait(): ordered by the Worker's mutex
    for (int i = 0; i < 200; i++) { w.run([&sum, i] { sum += i; }); w.wait(); }
    CHECK(sum == 199 * 200 / 2);
    w.run([] { throw std::runtime_error("job failed"); });
    bool threw = false;
    try { w.wait(); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    w.run([&sum] { sum = -1; }); w.wait();                       // the helper outlives a failed job, and the error is not reported twice
    CHECK(sum == -1);
    std::atomic<int> started{0}, finished{0};
    for (int i = 0; i < 20; i++) {                               // destruction with a job outstanding: a job that has started is finished before the destructor returns
        {
            hip_detail::Worker tmp;
            tmp.run([&] { started++; for (int k = 0; k < 50; k++) std::this_thread::yield(); finished++; });
            while (started.load() <= i) std::this_thread::yield();
        }
        CHECK(finished.load() == i + 1);
    }
    for (int i = 0; i < 20; i++) {                               // ... and one that has not started may be dropped, never run after its Worker is gone
        std::atomic<int> late{0};
        { hip_detail::Worker tmp; tmp.run([&late] { late++; }); }
        CHECK(late.load() <= 1);                                 // (late is gone after this line: a job that ran later would be a sanitizer report)
    }
    hip_detail::Worker* mine = hip_detail::thread_workers();
    hip_detail::Worker* theirs = nullptr;
    std::thread t([&] { theirs = hip_detail::thread_workers(); theirs[0].run([] {}); theirs[0].wait(); });
    t.join();
    CHECK(theirs && theirs != mine);
    return 0;
}

static int handle_section()
{
    const int T = 4;
    std::mutex mu; std::set<hs_orb*> seen; std::atomic<int> bad{0};
    Gate g(T), all_made(T); std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t] {
        g.arrive();
        hs_orb* h = hip_detail::thread_handle(0, "adaptor_threads");
        if (h != hip_detail::thread_handle(0, "adaptor_threads")) bad++;
        { std::lock_guard<std::mutex> l(mu); if (!seen.insert(h).second) bad++; }
        all_made.arrive();                                       // every handle is alive until here: no address can have been reused
        std::mt19937 rng(100 + t);
        for (int i = 0; i < 10 * (t + 1); i++) {                 // the threads finish one after the other: a handle is destroyed while the rest still work
            const int nq = 1 + (int)(rng() % 200), nt = 1 + (int)(rng() % 200);
            std::vector<uint8_t> q((size_t)nq * 32), tr((size_t)nt * 32); std::vector<int32_t> bi(nq), bd(nq), sd(nq);
            for (auto& v : q) v = (uint8_t)rng();
            if (hs_hamming_knn2(h, q.data(), nq, tr.data(), nt, bi.data(), bd.data(), sd.data()) != HS_OK) bad++;
        }
    });
    for (auto& t : th) t.join();
    CHECK(bad.load() == 0 && (int)seen.size() == T);
    return 0;
}

static int live_threads()
{
    int n = 0;
    if (DIR* d = opendir("/proc/self/task")) { while (dirent* e = readdir(d)) n += e->d_name[0] != '.'; closedir(d); }
    return n;
}

// helpers_seen: the helper threads the gathers really started, per calling thread (persistent Workers: they live as long as their caller)
static int gather_section(int& helpers_seen)
{
    std::map<std::string, FeatureExtractorSettings> per_type;
    per_type["SLAM"].nFeatures = 1000;
    FeatureMatcherSettings ms; ms.nnratio = 0.8f;
    std::unique_ptr<FeatureFactory> factory = std::make_unique<HipORBFactory>(per_type, ms, 0);
    std::shared_ptr<DescriptorDistance> dist = factory->getDistanceFunc();
    const int n_kp = 300, n_lm = 5000;
    std::mt19937 rng(7);
    std::vector<uint8_t> desc((size_t)n_kp * 32);
    for (auto& v : desc) v = (uint8_t)rng();
    std::vector<cv::KeyPoint> keys(n_kp); std::vector<FeatureDescriptor> descs; std::vector<float> uR(n_kp, -1.f), depth(n_kp, -1.f);
    for (int i = 0; i < n_kp; i++) {
        keys[i].pt.x = (float)(rng() % 640); keys[i].pt.y = (float)(rng() % 480); keys[i].size = 31.f; keys[i].angle = (float)(rng() % 360); keys[i].response = 30.f; keys[i].octave = (int)(rng() % 8);
        descs.push_back(FeatureDescriptor(cv::Mat(1, 32, CV_8UC1, desc.data() + (size_t)i * 32, 32), dist));
    }
    Camera cam; cam.sensor = 1;
    for (int i = 0; i < 9; i++) cam.K.at<float>(i / 3, i % 3) = 0.f;
    cam.K.at<float>(0, 0) = cam.K.at<float>(1, 1) = 500.f; cam.K.at<float>(0, 2) = 320.f; cam.K.at<float>(1, 2) = 240.f; cam.K.at<float>(2, 2) = 1.f;
    cam.mbf = 60.f; cam.mnMinX = 0; cam.mnMaxX = 640.f; cam.mnMinY = 0; cam.mnMaxY = 480.f;
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = r == c ? 1.f : 0.f;
    std::vector<MapPoint*> lm(n_lm, nullptr);
    for (int j = 0; j < n_lm; j++) {
        if (j % 97 == 0) continue;                               // null entries, as a local map has them
        MapPoint* m = new MapPoint();
        m->mWorldPos.at<float>(0) = (float)(rng() % 7) - 3.f; m->mWorldPos.at<float>(1) = (float)(rng() % 5) - 2.f; m->mWorldPos.at<float>(2) = 4.f + (float)(rng() % 6);
        m->mNormalVector.at<float>(0) = 0.f; m->mNormalVector.at<float>(1) = 0.f; m->mNormalVector.at<float>(2) = 1.f;
        m->size = 0.5f; m->mfMinDistance = 1.f; m->mfMaxDistance = 50.f; m->nObs = 1 + j % 3;
        m->mDescriptor = FeatureDescriptor(cv::Mat(1, 32, CV_8UC1, desc.data() + (size_t)(j % n_kp) * 32, 32), dist);
        lm[j] = m;
    }
    const FeatureExtractorSettings orb;
    std::atomic<int> bad{0}, base{-1}, after_small{-1}, after_large{-1};
    Gate g(2), searched_small(2), counted_small(2), searched_large(2), counted_large(2); std::vector<std::thread> th;
    for (int t = 0; t < 2; t++) th.emplace_back([&, t] {        // two calling threads (Tracking and a Mapping job): a frame, a matcher, a handle and helpers each
        g.arrive();
        try {
            Frame F(FeatureViews(keys, std::vector<cv::KeyPoint>(), uR, depth, descs, std::vector<FeatureDescriptor>(), orb), cam);
            F.SetPose(Tcw);
            for (int j = t; j < n_lm; j += 50) if (lm[j]) F.associateLandMark((j / 50) % n_kp, lm[j], true);
            std::unique_ptr<FeatureMatcher> matcher = factory->getFeatureMatcher();
            {   // which path the gather takes, seen from outside: 4095 landmarks start no helper, 4096 start them (they stay alive with their caller)
                std::vector<MapPoint*> distinct;
                for (MapPoint* p : lm) if (p) distinct.push_back(p);
                const std::vector<MapPoint*> below(distinct.begin(), distinct.begin() + 4095), at(distinct.begin(), distinct.begin() + 4096);
                if (t == 0) base = live_threads();               // (both callers exist: whatever else the process runs, a sanitizer's own thread for instance, is in it)
                hip_stub_zero_device();
                if (matcher->SearchByProjection(F, below, 5.f) < 0) bad++;
                searched_small.arrive(); if (t == 0) after_small = live_threads(); counted_small.arrive();
                hip_stub_zero_device();
                if (matcher->SearchByProjection(F, at, 5.f) < 0) bad++;
                searched_large.arrive(); if (t == 0) after_large = live_threads(); counted_large.arrive();
            }
            for (int rep = 0; rep < 6; rep++) {
                hip_stub_zero_device();                          // (no kernel writes the outputs: start every search from what a fresh allocation holds)
                const int n = matcher->SearchByProjection(F, lm, 5.f);
                if (n < 0) bad++;
                std::vector<MapPoint*> few(lm.begin(), lm.begin() + 4000);      // below the split: the calling thread gathers alone
                hip_stub_zero_device();                          // (or the "results" are what the last call uploaded: indices that are no views)
                if (matcher->SearchByProjection(F, few, 3.f) < 0) bad++;
            }
        } catch (const std::exception& e) { printf("thread %d: %s\n", t, e.what()); bad++; }
    });
    for (auto& t : th) t.join();
    for (MapPoint* m : lm) delete m;
    CHECK(bad.load() == 0);
    const char* e = std::getenv("HYSLAM_AMD_GATHER_THREADS");
    const int asked = e ? std::atoi(e) : 2;
    const int want = std::min<int>(std::min(asked, 2), (int)std::max(1u, std::thread::hardware_concurrency()) - 1);
    CHECK(base.load() >= 3 && after_small.load() == base.load());        // 4095 landmarks: nobody was started
    helpers_seen = (after_large.load() - base.load()) / 2;
    CHECK(after_large.load() == base.load() + 2 * want);                 // 4096: `want` helpers per calling thread
    return 0;
}

int main()
{
    setvbuf(stdout, nullptr, _IONBF, 0);
    int ndev = 0;
    CHECK(hs_device_count(&ndev) == HS_OK && ndev == 1);
    CHECK(worker_section() == 0);
    CHECK(handle_section() == 0);
    int helpers = -1;
    CHECK(gather_section(helpers) == 0);
    printf("ADAPTOR THREADS OK: Worker, thread_handle on 4 threads, 2 x 6 projection searches over 5000 landmarks, %d gather helper threads seen per caller\n", helpers);
    return 0;
}
