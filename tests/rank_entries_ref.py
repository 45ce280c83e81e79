"""
Restatement of csrk_rank_entries' rule 3 (include/csrk.h) for the tests: nothing here is shared with the library.  The scores
come from tests/topk_scores_ref.py (scores_exact, scores_plain, scores_two_rounding), and so does the order (key).

    ranks          for every test entry (i, j), in storage order, a plain count over the items c != j that `seen` does not
                   store in row i of those whose (key, item) comes before (key of s_ij, j): larger key first, on equal keys
                   the smaller item.
    entry_scores   S[i, j] for every test entry, in storage order.
"""
import numpy as np

from topk_scores_ref import key, scores_exact, scores_plain, scores_two_rounding      # noqa: F401  (re-exported for the tests)


def ranks(S, seen_rowptrs, seen_colinds, test_rowptrs, test_colinds):
    """
    int32 [number of test entries of the rows of S]; row r of S is row r of both patterns (seen_rowptrs None: nothing seen).
    """
    S = np.asarray(S, np.float64)
    m, n_items = S.shape
    items = np.arange(n_items)
    out = []
    for r in range(m):
        unseen = np.ones(n_items, bool)
        if seen_rowptrs is not None:
            unseen[np.asarray(seen_colinds[int(seen_rowptrs[r]):int(seen_rowptrs[r + 1])], np.int64)] = False
        K = key(S[r])
        for e in range(int(test_rowptrs[r]), int(test_rowptrs[r + 1])):
            j = int(test_colinds[e])
            before = (K > K[j]) | ((K == K[j]) & (items < j))
            before[j] = False                                     # c != j (it ties with itself anyway)
            out.append(int(np.count_nonzero(before & unseen)))
    return np.array(out, np.int32)


def entry_scores(S, test_rowptrs, test_colinds):
    S = np.asarray(S, np.float64)
    out = [S[r, int(test_colinds[e])] for r in range(S.shape[0]) for e in range(int(test_rowptrs[r]), int(test_rowptrs[r + 1]))]
    return np.array(out, np.float64)
