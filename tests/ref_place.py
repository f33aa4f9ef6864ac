"""Independent pure-Python restatement of hySLAM's place recognition, to be read line against line with the reference:

  bow_vector          DBoW2::TemplatedVocabulary::transform's BoW half: `if (w > 0) v.addWeight(id, w)` per feature, then v.normalize(L1)
  l1_score            DBoW2::L1Scoring::score — the merge over two sorted maps (FeatureVocabulary::score, ORBVocabulary.cpp:44-46)
  PlaceRecognizerRef  src/core/PlaceRecognizer.cpp:43-311 with its own structures: the inverted file is a list per word, the relocalisation query
                      keeps the "first encounter" list lKFsSharingWords, the loop query a dict walked in key order (std::map<KeyFrame*, int>)

A key frame is an integer key; it stands for the KeyFrame* and orders whatever the reference orders by address.  Python floats are
IEEE doubles; where the reference holds a `float` the value goes through numpy.float32.  One rule is not the reference's: the
relocalisation query reads pKF2->mRelocScore of ANY neighbour that shares a word, a field it only writes for key frames above minCommonWords — here
such a neighbour contributes the score it has.

`mutate` names a deliberate mistake (tests/test_place_ref.py shows that every one of them is caught)."""
from collections import Counter

import numpy as np

F32 = np.float32
MUTANTS = ("count_from_1", "ge", "double_product", "tree_sum", "key_order")


def bow_vector(word, weight, order="feature"):
    """-> (words ascending, values): per-word double sums of the float weights in FEATURE order, L1-normalised with the norm added in WORD order"""
    bow = {}
    idx = range(len(word))
    if order == "sorted":                                   # a wrong order, for the last-bit test
        idx = sorted(idx, key=lambda i: float(weight[i]))
    for i in idx:
        w = float(F32(weight[i]))
        if w > 0:                                           # if (w > 0) v.addWeight(id, w)
            wid = int(word[i])
            if wid in bow:
                bow[wid] += w
            else:
                bow[wid] = w
    norm = 0.0
    for wid in sorted(bow):                                 # BowVector::normalize(L1): the std::map's order
        norm += abs(bow[wid])
    words = sorted(bow)
    if norm > 0.0:
        return words, [bow[k] / norm for k in words]
    return words, [bow[k] for k in words]


def _tree_sum(terms):
    t = list(terms)
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0] if t else 0.0


def l1_score(v1, v2, mutate=None):
    """v1, v2: lists of (word, value) in ascending word order"""
    i, j, score, terms = 0, 0, 0.0, []
    while i < len(v1) and j < len(v2):
        if v1[i][0] == v2[j][0]:
            vi, wi = v1[i][1], v2[j][1]
            t = abs(vi - wi) - abs(vi) - abs(wi)
            terms.append(t)
            score += t
            i += 1
            j += 1
        elif v1[i][0] < v2[j][0]:
            i += 1                                          # (DBoW2 jumps with lower_bound; the visited pairs are the same)
        else:
            j += 1
    if mutate == "tree_sum":
        score = _tree_sum(terms)
    return -score / 2.0


class PlaceRecognizerRef:
    def __init__(self, n_words, mutate=None):
        assert mutate is None or mutate in MUTANTS
        self.n_words, self.mutate = n_words, mutate
        self.inverted = [[] for _ in range(n_words)]        # mvInvertedFile
        self.bow = {}                                       # key -> [(word, value)] ascending: pKF->mBowVec
        self.trace = Counter()                              # which branches a query took

    def add(self, key, words, values):
        assert key not in self.bow
        self.bow[key] = list(zip([int(w) for w in words], [float(v) for v in values]))
        for w, _ in self.bow[key]:
            self.inverted[w].append(key)

    def erase(self, key):
        for w, _ in self.bow[key]:
            self.inverted[w].remove(key)
        del self.bow[key]

    def clear(self):
        self.inverted = [[] for _ in range(self.n_words)]
        self.bow = {}

    def _min_common(self, max_common):
        if self.mutate == "double_product":
            return int(max_common * 0.8)
        return int(F32(max_common) * F32(0.8))              # int minCommonWords = maxCommonWords*0.8f

    def _gt(self, a, b):
        return a >= b if self.mutate == "ge" else a > b

    def _score(self, q, key):
        return F32(l1_score(q, self.bow[key], self.mutate))  # float si = mpVoc->score(...)

    def detect_reloc(self, qwords, qvalues, neigh):
        """neigh: key -> list of keys (GetBestCovisibilityKeyFrames(10)).  -> (candidates in ascending key order, details)"""
        q = list(zip([int(w) for w in qwords], [float(v) for v in qvalues]))
        sharing, reloc_words = [], {}                       # lKFsSharingWords; mnRelocWords of the key frames with mnRelocQuery == F->mnId
        for w, _ in q:
            for k in self.inverted[w]:
                if k not in reloc_words:
                    reloc_words[k] = 0
                    sharing.append(k)
                reloc_words[k] += 1
        det = dict(words=dict(reloc_words), score={k: self._score(q, k) for k in sharing}, acc={}, best={})
        if not sharing:
            return [], det
        max_common = 0
        for k in sharing:
            if reloc_words[k] > max_common:
                max_common = reloc_words[k]
        min_common = self._min_common(max_common)
        score_and_match = []
        for k in sharing:
            if self._gt(reloc_words[k], min_common):
                score_and_match.append((det["score"][k], k))
        if not score_and_match:
            return [], det
        acc_and_match, best_acc = [], F32(0)
        for si, k in score_and_match:
            best_score, acc, best = si, si, k
            for k2 in neigh.get(k, ()):
                if k2 not in self.bow:
                    self.trace["tombstone"] += 1            # erased: no longer in the inverted file, mnRelocQuery is stale
                    continue
                if k2 not in reloc_words:
                    continue
                s2 = det["score"][k2]                       # D9
                if not self._gt(reloc_words[k2], min_common):
                    self.trace["d9"] += 1
                acc = F32(acc + s2)
                if s2 > best_score:
                    best, best_score = k2, s2
                    self.trace["replace"] += 1
            det["acc"][k], det["best"][k] = acc, best
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(0.75) * best_acc
        added, out = set(), []
        for acc, best in acc_and_match:
            if self._gt(acc, retain):
                if best not in added:
                    out.append(best)
                    added.add(best)
                else:
                    self.trace["dedupe"] += 1
        return sorted(out), det                             # KeyFrameDB inserts them into a std::set<KeyFrame*>

    def detect_loop(self, qwords, qvalues, connected, min_score, neigh):
        q = list(zip([int(w) for w in qwords], [float(v) for v in qvalues]))
        connected, min_score = set(connected), F32(min_score)
        shared = {}                                         # std::map<KeyFrame*, int> shared_words
        for w, _ in q:
            for k in self.inverted[w]:
                if k in connected:
                    self.trace["excluded"] += 1
                    continue
                if k not in shared:
                    shared[k] = 1 if self.mutate == "count_from_1" else 0      # insert({pKFi, 0})
                else:
                    shared[k] += 1
        det = dict(words=dict(shared), score={k: self._score(q, k) for k in shared}, acc={}, best={})
        if not shared:
            return [], det
        walk = sorted(shared)                               # iteration order of the std::map
        max_common = 0
        for k in walk:
            if shared[k] > max_common:
                max_common = shared[k]
        min_common = self._min_common(max_common)
        score_and_match = []
        for k in walk:
            if self._gt(shared[k], min_common):
                si = det["score"][k]
                if si >= min_score:
                    score_and_match.append((si, k))
        if not score_and_match:
            return [], det
        acc_and_match, best_acc = [], min_score
        for si, k in score_and_match:
            best_score, acc, best = si, si, k
            for k2 in neigh.get(k, ()):
                if k2 not in self.bow:
                    self.trace["tombstone"] += 1
                    continue
                if k2 in shared and self._gt(shared[k2], min_common):
                    s2 = det["score"][k2]
                    acc = F32(acc + s2)
                    if s2 > best_score:
                        best, best_score = k2, s2
                        self.trace["replace"] += 1
            det["acc"][k], det["best"][k] = acc, best
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(0.75) * best_acc
        added, out = set(), []
        for acc, best in acc_and_match:
            if self._gt(acc, retain):
                if best not in added:
                    out.append(best)
                    added.add(best)
                else:
                    self.trace["dedupe"] += 1
        if self.mutate == "key_order":
            out = sorted(out)
        return out, det
