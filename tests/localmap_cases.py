"""Inputs for the local-map tests (tests/ref_localmap.py; hs_local_keyframes / hs_local_points): small cases whose answers are derived by hand from
src/slam/tracking/TrackLocalMap.cpp and written down, and seeded random ones."""
import numpy as np

from kfgraph_cases import random_table, table

N_KF = 6


def _kf(voted, n_max=80, n_neighbor=3, bad=(), neigh=None, parent=None):
    """six key frames, rows of three neighbours; voted: the slots with a positive count; neigh / parent: {slot: row} / {slot: parent}"""
    w = np.zeros(N_KF, np.int32)
    w[list(voted)] = 5
    b = np.zeros(N_KF, np.uint8)
    b[list(bad)] = 1
    ng = np.full((N_KF, 3), -1, np.int32)
    for s, row in (neigh or {}).items():
        ng[s, :len(row)] = row
    par = np.full(N_KF, -1, np.int32)
    for s, q in (parent or {}).items():
        par[s] = q
    return dict(weights=w, kf_bad=b, neigh=ng, parent=par, n_max=n_max, n_neighbor=n_neighbor)


# ---- key-frame expansion (:106-156): expected `local` as the list of member slots
KNOWN_KEYFRAMES = {
    # slot 3 is the only member; its parent 1 lies BELOW the cursor: inserted, and never visited (its neighbour 5 stays out) — the walk has ended anyway
    "parent_below_cursor": dict(_kf([3], neigh={1: [5]}, parent={3: 1}), local=[1, 3]),
    # a NEIGHBOUR inserted below the cursor is never visited either: visiting 2 inserts 1, the next member above 2 is 4; 1's neighbour 5 stays out
    "neighbour_below_cursor_not_visited": dict(_kf([2, 4], neigh={2: [1], 1: [5]}), local=[1, 2, 4]),
    # the parent 4 of slot 1 lies above the cursor, but the `break` at :153 has ended the walk: 4 is not visited, its neighbour 5 stays out
    "parent_above_cursor": dict(_kf([1], neigh={4: [5]}, parent={1: 4}), local=[1, 4]),
    # a neighbour inserted AHEAD of the cursor is visited later: 0 inserts 3, 3 is visited and inserts 5
    "neighbour_ahead_visited_later": dict(_kf([0], neigh={0: [3], 3: [5]}), local=[0, 3, 5]),
    # 3 members > n_max = 2 at the first member: nothing is added
    "size_above_n_max_at_first_member": dict(_kf([0, 1, 2], n_max=2, neigh={0: [4]}), local=[0, 1, 2]),
    # 2 > 2 is false at slot 0 (strict), which inserts 3; at slot 1 the CURRENT size 3 > 2 stops the walk: 4 stays out
    "size_reaches_n_max_after_insert": dict(_kf([0, 1], n_max=2, neigh={0: [3], 1: [4]}), local=[0, 1, 3]),
    # a row of bad key frames only, and a row of -1 only
    "row_all_bad_or_all_empty": dict(_kf([0, 1], bad=[2, 3], neigh={0: [2, 3]}), local=[0, 1]),
    # the first neighbour that is not bad, and no further
    "first_good_neighbour_only": dict(_kf([0], bad=[2], neigh={0: [2, 3, 4]}), local=[0, 3]),
    "n_neighbor_zero": dict(_kf([0], n_neighbor=0, neigh={0: [3]}), local=[0]),
    # only the first n_neighbor entries of the row are looked at: the first is bad, the good second one is beyond n_neighbor = 1
    "n_neighbor_limits_the_row": dict(_kf([0], n_neighbor=1, bad=[2], neigh={0: [2, 3]}), local=[0]),
    # insert(pParent) does not ask isBad()
    "bad_parent_is_inserted": dict(_kf([2], bad=[0], parent={2: 0}), local=[0, 2]),
    # a neighbour that is already a member is still "the first that is not bad": nothing new, the next one is not looked at
    "neighbour_already_member": dict(_kf([0, 3], neigh={0: [3, 4]}), local=[0, 3]),
    # keyframeCounter.empty(): the set stays empty whatever the parents are
    "no_votes": dict(_kf([], parent={0: 1, 2: 3}), local=[]),
    # only a bad key frame was counted: the set is empty and the walk has nothing to visit
    "only_a_bad_key_frame_voted": dict(_kf([2], bad=[2], parent={2: 0}, neigh={2: [1]}), local=[]),
}

# ---- landmark selection (:166-184, :55-67).  Four key frames; landmark 0: seen by 0 and 1;  1: seen by 1, BAD;  2: seen by 0;  3: no observation;
# 4: seen by 3;  5: seen by 2 and 3
POINTS_TABLE = table(4, [[0, 1], [1], [0], [], [3], [2, 3]], lm_bad=[0, 1, 0, 0, 0, 0])


def _pt(local, frame_lm, cap, frame_remove, sel, n_sel):
    return dict(local=np.asarray(local, np.uint8), frame_lm=np.asarray(frame_lm, np.int32), cap=cap, frame_remove=frame_remove, sel=sel, n_sel=n_sel)


KNOWN_POINTS = {
    # LMid 0 holds the bad landmark 1: removed, and 1 is not selected;  LMid 1 is null;  LMid 2 holds the good landmark 2: erased from the local map.
    # Landmarks 4 and 5 have no local observer, 3 has no observer at all: only 0 is left
    "associated_bad_removed_and_associated_good_excluded": _pt([1, 1, 0, 0], [1, -1, 2], 3, [1, 0, 0], [0, -1, -1], 1),
    # slot 3 is in the set only as a (bad) parent (KNOWN_KEYFRAMES bad_parent_is_inserted): the landmarks it alone observes are local
    "only_local_observer_is_the_bad_parent": _pt([0, 0, 0, 1], [], 2, [], [4, 5], 2),
    # every key frame is local: 1 is bad, 3 has an empty observation range
    "empty_observation_range": _pt([1, 1, 1, 1], [-1], 6, [0], [0, 2, 4, 5, -1, -1], 4),
    "n_sel_zero": _pt([0, 0, 0, 0], [0], 2, [0], [-1, -1], 0),
    # every candidate is already held by the frame
    "n_sel_zero_all_held": _pt([1, 1, 1, 1], [0, 2, 4, 5, 5], 2, [0, 0, 0, 0, 0], [-1, -1], 0),
    # n_sel keeps the full count
    "cap_smaller_than_n_sel": _pt([1, 1, 1, 1], [], 3, [], [0, 2, 4], 4),
    "cap_zero": _pt([1, 1, 1, 1], [], 0, [], [], 4),
}


def random_keyframes(seed, n_kf, neigh_cap=10, p_vote=0.2, p_bad=0.1, p_parent=0.03):
    """votes on a fifth of the slots, rows of 0 .. neigh_cap random neighbours padded with -1, a parent on few slots so that the walk goes on"""
    rng = np.random.default_rng(seed)
    w = (rng.random(n_kf) < p_vote) * rng.integers(1, 50, n_kf)
    ng = np.full((n_kf, neigh_cap), -1, np.int32)
    for s in range(n_kf):
        k = int(rng.integers(0, neigh_cap + 1))
        ng[s, :k] = rng.integers(0, n_kf, k)
    par = np.where(rng.random(n_kf) < p_parent, rng.integers(0, n_kf, n_kf), -1).astype(np.int32)
    n_local0 = int((w > 0).sum())
    return dict(weights=w.astype(np.int32), kf_bad=(rng.random(n_kf) < p_bad).astype(np.uint8), neigh=ng, parent=par,
                n_max=int(rng.choice([0, max(n_local0 - 1, 0), n_local0, n_local0 + 2, 80, -1])), n_neighbor=int(rng.integers(0, neigh_cap + 1)))


def random_points(seed, n_kf, L, max_obs=12, big=(), n_assoc=200, p_local=0.3):
    """a random observation table, a random local set and a frame that holds n_assoc entries: null ones, bad ones and one landmark held twice"""
    rng = np.random.default_rng(seed)
    T = random_table(seed, n_kf, L, max_obs=max_obs, big=big, p_bad_lm=0.1)
    local = (rng.random(n_kf) < p_local).astype(np.uint8)
    flm = rng.integers(0, L, n_assoc).astype(np.int32) if L else np.full(n_assoc, -1, np.int32)
    flm[rng.random(n_assoc) < 0.2] = -1
    if n_assoc > 2:
        flm[-1] = flm[0]
    return T, local, flm
