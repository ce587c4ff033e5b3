"""The weighted k-nearest-neighbour vote in fp64 NumPy on the CPU: the specification that include/cstp_hip.h states for
cstp_knn_vote, restated for the host and the GPU tests.

    slot j is live iff 0 <= idx[j] < ng;  w_j = exp((val_j - val_0) * inv_t);  score(c) = sum of w_j over the live slots of class
    c in slot order;  output: the n_top best distinct classes by (score descending, class id ascending), (-1, 0) where they run
    out.

RTOL: the fp32 vote differs from this fp64 one by at most about (k + 3 + |arg|max) * 2^-24 relative -- k - 1 additions, the
subtraction, the product with inv_t and expf's own rounding, and exp turning the argument's absolute error |arg| * 2^-24 into a
relative one -- which is 6e-6 at k <= 64 and |arg| <= 2 / 0.07.  1e-4 is that bound with an order of magnitude to spare.  It is
the rtol for ``score``, and a rank whose score lies within relative 1e-4 of a neighbouring rank's score is a NEAR TIE: the fp32
vote may order the two the other way round, so the tests leave such ranks out (and bound how many there may be).
"""
import numpy as np

RTOL = 1e-4
MAX_NEAR_TIE_SHARE = 0.02


def vote_ref(val, idx, g_labels, inv_t, n_top):
    """val, idx [nq, k], g_labels [ng] (array-likes) -> (pred int64 [nq, n_top], score fp64 [nq, n_top], near_tie bool
    [nq, n_top]).  near_tie[i, r]: rank r exists and its score lies within relative RTOL of the score of rank r - 1 or r + 1 in
    the row's full ranking (rank n_top counts as a neighbour of rank n_top - 1)."""
    val = np.asarray(val, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(g_labels, dtype=np.int64)
    nq, k = val.shape
    ng = labels.shape[0]
    pred = np.full((nq, n_top), -1, dtype=np.int64)
    score = np.zeros((nq, n_top), dtype=np.float64)
    near = np.zeros((nq, n_top), dtype=bool)
    for i in range(nq):
        sums = {}
        for j in range(k):
            if 0 <= idx[i, j] < ng:
                c = int(labels[idx[i, j]])
                sums[c] = sums.get(c, 0.0) + float(np.exp((val[i, j] - val[i, 0]) * inv_t))
        ranked = sorted(sums.items(), key=lambda cs: (-cs[1], cs[0]))
        for r, (c, s) in enumerate(ranked[:n_top]):
            pred[i, r], score[i, r] = c, s
            for nb in (r - 1, r + 1):
                if 0 <= nb < len(ranked) and abs(s - ranked[nb][1]) <= RTOL * max(s, ranked[nb][1]):
                    near[i, r] = True
    return pred, score, near
