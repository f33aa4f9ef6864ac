// Single-thread CPU restatement of PlaceRecognizer's relocalisation query in the reference's own data structures — an inverted file of
// std::list<KeyFrame*> per word, the "first encounter" list, DBoW2's L1 score as a merge over two std::map<WordId, double>, the covisibility
// accumulation and the 0.75 retain test — written from the algorithm, as the comparison object of tools/bench_place.py.
// usage: place_walk_cpu db.bin repeats
//   db.bin  int32 n_words, n_kf; int64 offsets[n_kf+1]; int32 word[]; double value[]; int32 neigh[n_kf][10];
//           int32 n_queries; per query: int32 m, int32 word[m], double value[m]
// prints one line per query: "query i: <median us> us (min <..> max <..>) <n> candidates"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <vector>

struct KeyFrame {
    std::map<unsigned, double> bow;
    std::vector<KeyFrame*> neigh;
    long reloc_query = -1; int reloc_words = 0; float reloc_score = 0.f;
    int id = 0;
};

static double l1_score(const std::map<unsigned, double>& a, const std::map<unsigned, double>& b)
{
    auto i = a.begin(), j = b.begin();
    double s = 0;
    while (i != a.end() && j != b.end()) {
        if (i->first == j->first) { s += std::fabs(i->second - j->second) - std::fabs(i->second) - std::fabs(j->second); ++i; ++j; }
        else if (i->first < j->first) i = a.lower_bound(j->first);
        else j = b.lower_bound(i->first);
    }
    return -s / 2.0;
}

static std::vector<KeyFrame*> detect_reloc(std::vector<std::list<KeyFrame*>>& inverted, const std::map<unsigned, double>& q, long query_id)
{
    std::list<KeyFrame*> sharing;
    for (const auto& wv : q)
        for (KeyFrame* kf : inverted[wv.first]) {
            if (kf->reloc_query != query_id) { kf->reloc_words = 0; kf->reloc_query = query_id; kf->reloc_score = 0.f; sharing.push_back(kf); }
            kf->reloc_words++;
        }
    if (sharing.empty()) return {};
    int max_common = 0;
    for (KeyFrame* kf : sharing) max_common = std::max(max_common, kf->reloc_words);
    const int min_common = max_common * 0.8f;
    std::list<std::pair<float, KeyFrame*>> scored;
    for (KeyFrame* kf : sharing)
        if (kf->reloc_words > min_common) { kf->reloc_score = (float)l1_score(q, kf->bow); scored.push_back({kf->reloc_score, kf}); }
    if (scored.empty()) return {};
    std::list<std::pair<float, KeyFrame*>> acc;
    float best_acc = 0;
    for (auto& sk : scored) {
        float best = sk.first, a = sk.first;
        KeyFrame* bkf = sk.second;
        for (KeyFrame* n : sk.second->neigh) {
            if (n->reloc_query != query_id) continue;
            a += n->reloc_score;                       // (an unscored neighbour adds 0 here; the device adds the score it has, DESIGN.md D9: more work, not less)
            if (n->reloc_score > best) { bkf = n; best = n->reloc_score; }
        }
        acc.push_back({a, bkf});
        best_acc = std::max(best_acc, a);
    }
    const float retain = 0.75f * best_acc;
    std::set<KeyFrame*> seen;
    std::vector<KeyFrame*> out;
    for (auto& ak : acc) if (ak.first > retain && seen.insert(ak.second).second) out.push_back(ak.second);
    return out;
}

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: place_walk_cpu db.bin repeats\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int repeats = atoi(argv[2]);
    int32_t n_words, n_kf;
    rd(f, &n_words, 1); rd(f, &n_kf, 1);
    std::vector<int64_t> off((size_t)n_kf + 1);
    rd(f, off.data(), off.size());
    std::vector<int32_t> word((size_t)off[n_kf]);
    std::vector<double> value((size_t)off[n_kf]);
    rd(f, word.data(), word.size()); rd(f, value.data(), value.size());
    std::vector<int32_t> neigh((size_t)n_kf * 10);
    rd(f, neigh.data(), neigh.size());
    std::vector<KeyFrame> kfs((size_t)n_kf);
    std::vector<std::list<KeyFrame*>> inverted((size_t)n_words);
    for (int i = 0; i < n_kf; i++) {
        kfs[i].id = i;
        for (int64_t k = off[i]; k < off[i + 1]; k++) { kfs[i].bow[(unsigned)word[k]] = value[k]; inverted[word[k]].push_back(&kfs[i]); }
        for (int k = 0; k < 10; k++) { const int n = neigh[(size_t)i * 10 + k]; if (n >= 0 && n < n_kf) kfs[i].neigh.push_back(&kfs[n]); }
    }
    int32_t n_queries;
    rd(f, &n_queries, 1);
    long qid = 0;
    for (int qi = 0; qi < n_queries; qi++) {
        int32_t m;
        rd(f, &m, 1);
        std::vector<int32_t> qw((size_t)m); std::vector<double> qv((size_t)m);
        rd(f, qw.data(), qw.size()); rd(f, qv.data(), qv.size());
        std::map<unsigned, double> q;
        for (int i = 0; i < m; i++) q[(unsigned)qw[i]] = qv[i];
        std::vector<double> us;
        size_t n_out = 0;
        detect_reloc(inverted, q, qid++);                                      // warm-up
        for (int r = 0; r < repeats; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            n_out = detect_reloc(inverted, q, qid++).size();
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(us.begin(), us.end());
        printf("query %d: %.1f us (min %.1f max %.1f) %zu candidates\n", qi, us[us.size() / 2], us.front(), us.back(), n_out);
    }
    fclose(f);
    return 0;
}
