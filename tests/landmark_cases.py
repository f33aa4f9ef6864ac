"""Hand-built landmarks with known representative descriptors (MapPointDB.cpp:128-175), shared by the CPU and GPU landmark tests.
on_line(xs): descriptor k has its first xs[k] bits set, so distance(k, l) = |xs[k] - xs[l]| — the rows of the distance matrix are points on a line."""
import numpy as np


def prefix(n):
    bits = np.zeros(256, np.uint8)
    bits[:n] = 1
    return np.packbits(bits)


def on_line(xs):
    return np.stack([prefix(x) for x in xs]) if len(xs) else np.zeros((0, 32), np.uint8)


# name -> (descriptors, expected best, expected median)
KNOWN = {
    "n1": (on_line([37]), 0, 0),
    # N = 2: the median index is int(0.5) = 0, the diagonal 0 of both rows
    "n2": (on_line([0, 200]), 0, 0),
    # N = 3, index 1: rows [0,20,30] [0,10,30] [0,10,20] -> medians 20, 10, 10; the first of the tied rows wins
    "n3": (on_line([30, 0, 10]), 1, 10),
    # N = 4, index int(1.5) = 1 (the lower median): rows [0,10,11,13] [0,1,3,10] [0,1,2,11] [0,2,3,13] -> medians 10, 1, 1, 2: row 1.
    # With index N/2 = 2 the medians would be 11, 3, 2, 3 (row 2, median 2); with `<=` the tie of rows 1 and 2 would go to row 2.
    "n4_lower_median": (on_line([0, 10, 11, 13]), 1, 1),
    "identical": (np.tile(prefix(77), (5, 1)), 0, 0),
    # ties: rows [0,5,6,11] [0,1,5,6] [0,1,5,6] [0,5,6,11] -> medians 5, 1, 1, 5: the first of rows 1 and 2
    "tie_first_wins": (on_line([0, 5, 6, 11]), 1, 1),
    # the mean picks row 2 (row sums 106, 103, 102, 103, 394), the median picks row 1 (medians 2, 1, 1, 2, 98)
    "mean_vs_median": (on_line([0, 1, 2, 3, 100]), 1, 1),
    # N = 6, index int(2.5) = 2.  Sorted rows: [0,8,10,10,15,15] [0,5,5,15,23,30] [0,7,8,8,18,23] [0,7,15,15,25,30] [0,0,5,10,18,25] (x2)
    # -> medians 10, 5, 8, 15, 5, 5: row 1.  Index 3 would pick row 0 (median 10), index 1 row 4 (median 0), and `<=` row 5.
    "n6_index_and_strict": (on_line([21, 6, 29, 36, 11, 11]), 1, 5),
    # duplicates: two copies of a far descriptor, three of a near one
    "duplicates": (on_line([200, 3, 200, 3, 3]), 1, 0),
    # a complement: row 0 is [0, 256, 256] (median 256), rows 1 and 2 [0, 0, 256] (median 0)
    "complement": (np.stack([prefix(0), prefix(256), prefix(256)]), 1, 0),
}
