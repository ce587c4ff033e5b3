"""Few-shot episodes restated in fp64 with numpy: the specification that ops.fewshot_episodes and cstp_amd.fewshot are held to.
It never imports the code under test.

For episode e, shot count k and class slot c, with xs / xq the fp32 rows as given (widened, not re-normalised):

    p                 = sum_{j < k} xs[sup_idx[e, c, j]]              the FIRST k support columns
    score[s, e, q, c] = (xq[qry_idx[e, q]] . p) / |p|                 0 where |p| = 0
    pred[s, e, q]     = argmax_c score, the lowest slot on a tie
    hits[s, e]        = #{q : pred[s, e, q] == q // Q}
    margin[s, e, q]   = best score - second best score (fp64): how far a decision is from flipping

``make_features`` is the generator of the tests: class c has a random unit direction m_c, a row is 0.25 m_c + N(0, I / d), cast to
fp32 and normalised.  ``tol(d, kmax)`` is the bar of the GPU test: 2 (2 d + kmax + 8) 2^-24, the worst-case fp32 bound for
forming p, a length-d dot product, a length-d norm and one divide on operands whose exact score is at most 1 in magnitude.
"""
import functools

import numpy as np

N_CLASSES, PER_CLASS = 24, 40          # per list: 960 support rows, 960 query rows

# (d, N, shots, Q, E): d at and around the 128-feature slice (1, 3, 16 inside one; 255 / 256 / 257 / 513 at the edges of the
# second, third and fifth), both parities of the class-slot split (2, 5, 20 ways), 1 to 4 shot counts up to the limit of 16, 1 to
# 32 queries up to the limit of 320 slots, 1 to 40 episodes
CASES = [(1, 2, (1,), 1, 1), (3, 5, (1, 5), 15, 3), (16, 20, (1, 5, 16), 16, 20), (255, 5, (1, 5), 15, 40), (256, 2, (5,), 32, 20),
         (257, 20, (16,), 16, 20), (513, 5, (1, 2, 3, 4), 15, 40)]
GRID_CASE = (16, 2, (1,), 1, 70000)    # more blocks than 65 535: the grid dimension; 700 distinct episodes, tiled
GRID_DISTINCT = 700


def tol(d, kmax):
    return 2.0 * (2 * d + kmax + 8) * 2.0 ** -24


def make_features(d, seed, part=0, n_classes=N_CLASSES, per_class=PER_CLASS):
    """-> (x [n_classes * per_class, d] fp32 with unit rows, labels [n] int64), rows in a random order.  The class directions
    depend on ``seed`` alone; ``part`` (0: the support list, 1: the query list) draws other rows around the same directions."""
    m = np.random.default_rng(seed).standard_normal((n_classes, d))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    rng = np.random.default_rng([seed, part + 1])
    labels = rng.permutation(np.repeat(np.arange(n_classes), per_class))
    x = (0.25 * m[labels] + rng.standard_normal((len(labels), d)) / np.sqrt(d)).astype(np.float32)
    x = (x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return x, labels.astype(np.int64)


def make_tables(sup_labels, qry_labels, n_way, kmax, n_query, episodes, seed):
    """A plain sampler of the tests' own: per episode n_way distinct classes, per class kmax distinct support rows and n_query
    distinct query rows -> (sup_idx [E, N, kmax], qry_idx [E, N, Q]) int32."""
    rng = np.random.default_rng(seed)
    classes = np.unique(sup_labels)
    sup = np.empty((episodes, n_way, kmax), dtype=np.int32)
    qry = np.empty((episodes, n_way, n_query), dtype=np.int32)
    for e in range(episodes):
        for slot, c in enumerate(rng.choice(classes, n_way, replace=False)):
            sup[e, slot] = rng.choice(np.nonzero(sup_labels == c)[0], kmax, replace=False)
            qry[e, slot] = rng.choice(np.nonzero(qry_labels == c)[0], n_query, replace=False)
    return sup, qry


@functools.lru_cache(maxsize=None)
def case_data(d, n, shots, q, e):
    """The inputs and the reference of one case, computed once per process and shared (treat as read-only):
    -> (xs, xq, sup_idx, qry_idx, (score, pred, hits, margin))."""
    xs, ls = make_features(d, seed=d, part=0)
    xq, lq = make_features(d, seed=d, part=1)
    sup, qry = make_tables(ls, lq, n, shots[-1], q, e, seed=d + n)
    return xs, xq, sup, qry, episodes_ref(xs, xq, sup, qry, shots)


def episodes_ref(xs, xq, sup_idx, qry_idx, shots):
    """-> (score [S, E, N Q, N] fp64, pred [S, E, N Q] int32, hits [S, E] int32, margin [S, E, N Q] fp64)."""
    xs, xq = np.asarray(xs, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    e, n, _ = sup_idx.shape
    q = qry_idx.shape[2]
    prefix = np.cumsum(xs[sup_idx], axis=2)                               # [E, N, Kmax, d]: column order
    queries = xq[qry_idx.reshape(e, n * q)]                               # [E, N Q, d]
    score = np.zeros((len(shots), e, n * q, n))
    for s, k in enumerate(shots):
        p = prefix[:, :, k - 1, :]                                        # [E, N, d]
        norm = np.linalg.norm(p, axis=2)                                  # [E, N]
        dots = np.einsum("eqd,ecd->eqc", queries, p)
        score[s] = np.where(norm[:, None, :] > 0, dots / np.where(norm > 0, norm, 1.0)[:, None, :], 0.0)
    pred = score.argmax(axis=3).astype(np.int32)                          # numpy's argmax: the first of equal maxima
    own = (np.arange(n * q) // q)[None, None, :]
    hits = (pred == own).sum(axis=2).astype(np.int32)
    top2 = np.sort(score, axis=3)[..., -2:]
    return score, pred, hits, top2[..., 1] - top2[..., 0]


def episodes_loops(xs, xq, sup_idx, qry_idx, shots):
    """The same by the definition, one scalar at a time (for the specification's own test) -> (score, pred, hits)."""
    e_n, n, _ = sup_idx.shape
    q_n = qry_idx.shape[2]
    score = np.zeros((len(shots), e_n, n * q_n, n))
    pred = np.zeros((len(shots), e_n, n * q_n), dtype=np.int32)
    hits = np.zeros((len(shots), e_n), dtype=np.int32)
    for s, k in enumerate(shots):
        for e in range(e_n):
            for c in range(n):
                p = np.zeros(xs.shape[1])
                for j in range(k):
                    p = p + xs[sup_idx[e, c, j]].astype(np.float64)
                norm = float(np.sqrt((p * p).sum()))
                for q in range(n * q_n):
                    row = xq[qry_idx[e, q // q_n, q % q_n]].astype(np.float64)
                    score[s, e, q, c] = float((row * p).sum()) / norm if norm > 0 else 0.0
            for q in range(n * q_n):
                best = 0
                for c in range(1, n):
                    if score[s, e, q, c] > score[s, e, q, best]:
                        best = c
                pred[s, e, q] = best
                hits[s, e] += int(best == q // q_n)
    return score, pred, hits
