"""Cases for the place-recognition tests: hand-derived ones (values are powers of two, so every expected number below is exact) and seeded
scenes.  A case is a dict: mode ("reloc" / "loop"), entries [(key, words, values)] in add order, erased [keys], query (words, values), neigh
{key: [keys]}, connected [keys], min_score, expect (the candidate keys), and optionally expected words / score / acc / best by key."""
import numpy as np

N_WORDS = 1000


def vec(shared, fill_from=None, n=32, value=None):
    """`n` words: the words of `shared` (a range or list), padded with private words from `fill_from`; every value 1/n unless given"""
    w = list(shared)
    k = fill_from
    while len(w) < n:
        w.append(k)
        k += 1
    w = sorted(w)
    return w, [1.0 / n if value is None else value] * len(w)


Q32 = vec(range(32))            # the usual query: words 0..31, 1/32 each; a key frame sharing k of them (equal values) scores k/32


def kf(key, k_shared, fill_from):
    return (key,) + vec(range(k_shared), fill_from)


def _case(mode, entries, query, expect, **kw):
    c = dict(mode=mode, entries=entries, query=query, expect=expect, neigh={}, connected=[], min_score=0.0, erased=[])
    c.update(kw)
    return c


T = 2.0 ** -53
KNOWN = {
    # 4 shared words of 1/4: every term |0| - 1/4 - 1/4, sum -2, score 1
    "identical_reloc": _case("reloc", [(7, [1, 2, 3, 4], [0.25] * 4)], ([1, 2, 3, 4], [0.25] * 4), [7], words={7: 4}, score={7: 1.0}, acc={7: 1.0}, best={7: 7}),
    # loop count 3, minCommonWords = int(2.4f) = 2; si = 1 >= 0.5; acc 1 > 0.75 * max(0.5, 1)
    "identical_loop": _case("loop", [(7, [1, 2, 3, 4], [0.25] * 4)], ([1, 2, 3, 4], [0.25] * 4), [7], min_score=0.5, words={7: 3}, score={7: 1.0}),
    "disjoint": _case("reloc", [(7, [1, 2], [0.5, 0.5]), (9, [10, 11], [0.5, 0.5])], ([10, 11], [0.5, 0.5]), [9], words={9: 2}, score={9: 1.0}),
    "nothing_shared": _case("reloc", [(7, [1, 2], [0.5, 0.5]), (9, [10, 11], [0.5, 0.5])], ([20, 21], [0.5, 0.5]), [], words={}),
    "nothing_shared_loop": _case("loop", [(7, [1, 2], [0.5, 0.5])], ([20, 21], [0.5, 0.5]), [], words={}),
    # one shared word: the loop query's count is 0, maxCommonWords 0, nothing is scored; the relocalisation query counts 1
    "one_word_loop": _case("loop", [(3, [1], [1.0])], ([1], [1.0]), [], words={3: 0}, score={3: 1.0}),
    "one_word_reloc": _case("reloc", [(3, [1], [1.0])], ([1], [1.0]), [3], words={3: 1}, score={3: 1.0}),
    # maxCommonWords 5 -> minCommonWords 4: the key frame with 4 shared words is not scored (it would be retained: 4/32 > 0.75 * 5/32)
    "trunc_5": _case("reloc", [kf(1, 5, 100), kf(2, 4, 200)], Q32, [1], words={1: 5, 2: 4}, best={1: 1}),
    # 10 -> 8: 9 is scored, 8 is not
    "trunc_10": _case("reloc", [kf(1, 10, 100), kf(2, 8, 200), kf(3, 9, 300)], Q32, [1, 3], words={1: 10, 2: 8, 3: 9}),
    # counts 25, 25, 26 (shared 26, 26, 27), minCommonWords int(20.8f) = 20.  Entry 10: neighbour 40 scores more -> pBestKF 40, acc 26/32 + 27/32.
    # Entry 20: neighbour 10 scores the same -> keeps itself, acc 52/32.  Entry 40: neighbour 20, acc 53/32.  retain 0.75 * 53/32: all three
    # retained; the walk (keys 10, 20, 40) gives 40, 20, 40 -> [40, 20], which is not ascending key order
    "replace_dedupe_walk": _case("loop", [kf(10, 26, 100), kf(20, 26, 200), kf(40, 27, 300)], Q32, [40, 20], min_score=0.5,
                                 neigh={10: [40], 20: [10], 40: [20]}, words={10: 25, 20: 25, 40: 26},
                                 acc={10: 53 / 32, 20: 52 / 32, 40: 53 / 32}, best={10: 40, 20: 20, 40: 40}),
    # the same scene through the relocalisation query: the set {40, 20} in ascending key order
    "replace_dedupe_reloc": _case("reloc", [kf(10, 26, 100), kf(20, 26, 200), kf(40, 27, 300)], Q32, [20, 40],
                                  neigh={10: [40], 20: [10], 40: [20]}, words={10: 26, 20: 26, 40: 27}, best={10: 40, 20: 20, 40: 40}),
    # key frame 2 shares 26 words, 22 of them with 1/32 and 4 with 1/64: si = 22/32 + 4/64 = 0.75 = 0.75f * bestAccScore exactly: not retained
    "acc_at_threshold": _case("reloc", [kf(1, 32, 100), (2, list(range(26)) + list(range(200, 206)), [1 / 32] * 22 + [1 / 64] * 4 + [1 / 32] * 6)], Q32, [1],
                              words={1: 32, 2: 26}, score={1: 1.0, 2: 0.75}, acc={1: 1.0, 2: 0.75}),
    # si == minScore is listed (>=)
    "score_equals_min_score": _case("loop", [kf(1, 32, 100), kf(2, 28, 200)], Q32, [1], min_score=1.0, words={1: 31, 2: 27}, score={1: 1.0, 2: 0.875},
                                    best={1: 1, 2: -1}),
    # connected key frame 1 would have won; without it maxCommonWords drops from 31 to 27, minCommonWords from 24 to 21, and key frame 3
    # (count 22, si 23/32 > 0.75 * 28/32) comes in
    "excluded_winner": _case("loop", [kf(1, 32, 100), kf(2, 28, 200), kf(3, 23, 300)], Q32, [2, 3], connected=[1], min_score=0.5, words={2: 27, 3: 22}),
    "not_excluded": _case("loop", [kf(1, 32, 100), kf(2, 28, 200), kf(3, 23, 300)], Q32, [1, 2], min_score=0.5, words={1: 31, 2: 27, 3: 22}),
    # the erased key frame 9 (identical to the query) is key frame 1's neighbour: ignored
    "tombstoned_neighbour": _case("reloc", [kf(1, 26, 100), kf(9, 32, 200)], Q32, [1], erased=[9], neigh={1: [9]}, words={1: 26}, acc={1: 26 / 32}, best={1: 1}),
    # D9: neighbour 5 shares 4 words (not scored: 4 <= 25) and still adds its 4/32: acc 36/32, retain 27/32 = key frame 2's acc: not retained
    # (without the neighbour's score key frame 2 would be a candidate)
    "d9_neighbour": _case("reloc", [kf(1, 32, 100), kf(2, 27, 200), kf(5, 4, 300)], Q32, [1], neigh={1: [5]}, words={1: 32, 2: 27, 5: 4},
                          score={5: 0.125}, acc={1: 1.125, 2: 27 / 32}, best={1: 1}),
    # the ordered double sum: terms -(2 + 2^-23), -2^-52, -2^-52, -2^-52.  Left to right every -2^-52 is half an ulp and ties to even: s = -(2 + 2^-23),
    # score 1 + 2^-24, a float tie -> 1.0f.  A pairwise sum adds 2^-51 at once: score 1 + 2^-24 + 2^-52 -> 1 + 2^-23
    "ordered_score_sum": _case("reloc", [(1, [0, 1, 2, 3], [1 + 2.0 ** -24, T, T, T])], ([0, 1, 2, 3], [1 + 2.0 ** -24, T, T, T]), [1], words={1: 4}, score={1: 1.0}),
}

# BoW vector: word 5 gets 1.0 + 2^-53 + 2^-53 in feature order = 1.0 (each addend is half an ulp, ties to even); in ascending-weight order it is
# 1 + 2^-52, the norm 2 + 2^-52 rounds to 2, and the value becomes 0.5 + 2^-53.  The feature with weight 0 is left out.
BOW_LAST_BIT = dict(word=[5, 9, 5, 3, 5], weight=[1.0, 1.0, T, 0.0, T], expect=([5, 9], [0.5, 0.5]), sorted_expect=([5, 9], [0.5 + T, 0.5]))


def run_ref(R, case, mutate=None, n_words=N_WORDS):
    ref = R.PlaceRecognizerRef(n_words, mutate)
    for key, w, v in case["entries"]:
        ref.add(key, w, v)
    for key in case["erased"]:
        ref.erase(key)
    qw, qv = case["query"]
    if case["mode"] == "reloc":
        out, det = ref.detect_reloc(qw, qv, case["neigh"])
    else:
        out, det = ref.detect_loop(qw, qv, case["connected"], case["min_score"], case["neigh"])
    return out, det, ref


def random_scene(seed, n_kf, n_words, lens=(5, 60), big=(), n_queries=6, erase=0.03):
    """A seeded database of `n_kf` key frames in "places" of ~6 consecutive key frames that share most of their words (every place comes twice), with keys in an order
    unrelated to the slots, covisibility lists inside and across places, a few erased key frames, and queries that are perturbed copies of
    stored vectors.  big: [(index, length)].  -> dict(entries, erased, neigh, queries=[case-like dicts])"""
    rng = np.random.default_rng(seed)
    hi = min(lens[1], n_words)
    n_places = max(1, n_kf // 6)
    base = [rng.choice(n_words, size=hi, replace=False) for _ in range(n_places)]
    keys = (rng.permutation(n_kf).astype(np.int64) * 7919 + 1000).tolist()
    big = dict(big)
    place_len = rng.integers(lens[0], hi + 1, n_places)    # the key frames of a place are about as long as each other
    half = n_places // 2                                   # every place is visited twice, far apart in the sequence (a loop to close)
    for pl in range(half, 2 * half):
        base[pl], place_len[pl] = base[pl - half], place_len[pl - half]
    entries = []
    for i in range(n_kf):
        L = min(int(big.get(i, place_len[min(i // 6, n_places - 1)])), n_words)
        b = base[min(i // 6, n_places - 1)]
        n_take = min(len(b), L, int(round(0.95 * L))) if rng.random() < 0.95 else 0
        chosen = set(b[:n_take].tolist())
        for x in rng.choice(n_words, size=L, replace=False).tolist():      # private words up to the length
            if len(chosen) >= L:
                break
            chosen.add(x)
        w = np.array(sorted(chosen), np.int32)
        v = rng.random(len(w)) * 0.2 + 0.9
        entries.append((keys[i], w.astype(np.int32), v / v.sum()))
    erased = [keys[i] for i in np.nonzero(rng.random(n_kf) < erase)[0]] if n_kf > 2 else []
    neigh = {}
    for i in range(n_kf):
        pl = min(i // 6, n_places - 1)
        if rng.random() < 0.9:                              # the other key frames of this visit of the place, then a few from elsewhere
            lo = next(j for j in range(max(0, i - 8), i + 1) if min(j // 6, n_places - 1) == pl)
            mates = [j for j in range(lo, min(n_kf, lo + 12)) if min(j // 6, n_places - 1) == pl and j != i]
            r = i % max(len(mates), 1)
            pick = (mates[r:] + mates[:r] + rng.integers(0, n_kf, int(rng.integers(0, 3))).tolist())[:10]
        else:
            cnt = int(rng.integers(0, 11))
            near = np.clip(i + rng.integers(-6, 7, cnt), 0, n_kf - 1)
            pick = np.where(rng.random(cnt) < 0.85, near, rng.integers(0, n_kf, cnt)).tolist()
        neigh[keys[i]] = [keys[j] for j in pick if j != i]
    live = [i for i in range(n_kf) if keys[i] not in set(erased)] or [0]
    queries = []
    for qi in range(n_queries):
        j = live[int(rng.integers(0, len(live)))]
        w0 = entries[j][1]
        keep = w0[rng.random(len(w0)) < 0.9]
        w = np.unique(np.concatenate([keep, rng.choice(n_words, size=max(1, len(w0) // 8), replace=False)])).astype(np.int32)
        v = rng.random(len(w)) + 0.05
        q = dict(mode="loop" if qi % 2 else "reloc", query=(w, v / v.sum()), connected=[], min_score=0.0)
        if q["mode"] == "loop":
            q["connected"] = [k for k in neigh[keys[j]][:int(rng.integers(0, 4))]] + ([keys[j]] if rng.random() < 0.3 else [])
            q["min_score"] = float(np.float32(rng.choice([0.0, 0.02, 0.1])))
        queries.append(q)
    return dict(entries=entries, erased=erased, neigh=neigh, queries=queries, n_words=n_words)


def scene_ref(R, scene):
    ref = R.PlaceRecognizerRef(scene["n_words"])
    for key, w, v in scene["entries"]:
        ref.add(key, w, v)
    for key in scene["erased"]:
        ref.erase(key)
    return ref


def ref_query(ref, scene, q):
    if q["mode"] == "reloc":
        return ref.detect_reloc(q["query"][0], q["query"][1], scene["neigh"])
    return ref.detect_loop(q["query"][0], q["query"][1], q["connected"], q["min_score"], scene["neigh"])


# the seeded set of tests/test_gpu_place.py: (seed, key frames, vocabulary words, length range, [(index, length)], queries).  The seeds are chosen so
# that the conditions of tests/test_place_ref.py::test_seeded_scenes_meet_their_conditions hold.
SCENES = [
    (1, 1, 1000, (5, 60), [], 2),
    (2, 2, 1000, (5, 60), [], 2),
    (9, 500, 1000, (5, 60), [(7, 1), (8, 63), (9, 64), (10, 65), (11, 128), (12, 129), (13, 1000)], 12),
    (11, 500, 1000000, (20, 200), [(3, 1), (4, 64), (5, 65), (6, 4097), (7, 10000)], 12),
    (5, 20000, 1000, (5, 60), [(100, 64), (101, 65), (19999, 700)], 4),
    (6, 20000, 1000000, (20, 120), [(5, 10000), (6, 2048), (7, 2049)], 4),
]


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def trained_vocab_tree(cls, descs, k, levels, seed):
    """A vocabulary built from real descriptors, as DBoW2's are (random node descriptors do not group the descriptors of real images): every node's
    children are `k` of the descriptors that reached it (seeded choice), the others go to their nearest child; leaves carry consecutive word ids
    and the idf weight log(N / N_word).  -> (cls instance, keepalive arrays, number of words)"""
    rng = np.random.default_rng(seed)
    descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    cb, cc, nd, members, level = [0], [0], [np.zeros(32, np.uint8)], [np.arange(len(descs))], [0]
    i = 0
    while i < len(nd):
        m = members[i]
        if level[i] < levels and len(m) >= k:
            pick = m[rng.choice(len(m), k, replace=False)]
            nearest = _POP[descs[m][:, None, :] ^ descs[pick][None, :, :]].sum(2).argmin(1)
            cb[i], cc[i] = len(nd), k
            for c in range(k):
                nd.append(descs[pick[c]]); cb.append(0); cc.append(0); members.append(m[nearest == c]); level.append(level[i] + 1)
        i += 1
    n = len(nd)
    cb, cc, desc = np.array(cb, np.int32), np.array(cc, np.int32), np.array(nd, np.uint8)
    leaf = cc == 0
    leaf[0] = False
    word = np.full(n, -1, np.int32)
    word[leaf] = np.arange(leaf.sum())
    weight = np.zeros(n, np.float32)
    count = np.array([len(m) for m in members])
    weight[leaf] = (np.log((len(descs) + 1.0) / (count[leaf] + 1.0)) + 0.1).astype(np.float32)
    return cls(n, levels, cb.ctypes.data, cc.ctypes.data, desc.ctypes.data, word.ctypes.data, weight.ctypes.data, None), [cb, cc, desc, word, weight], int(leaf.sum())
