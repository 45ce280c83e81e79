"""
The listed-rows steps of the host forms csrk_topk_scores_for and csrk_rank_entries_for on the card (csrc/score_host.h:
check_listed_rows, pack_listed_rows), where the caller's stride and the list meet: U a strided view (ldu = k + 3), the list
(4, 0, 4) out of 5 rows, 129 items -- two tiles and one item, so that two splits sweep uneven ranges and three leave a range of
one item --, k = 4 (16-byte loads on the packed copy) and k = 5 (element loads), float32 and float64, splits automatic, 1, 2
and 3, with and without `seen`.  Bit for bit against tests/topk_scores_ref.py and tests/rank_entries_ref.py on the gathered
rows, and equal to the range entries over rows (0, 5) picked at rows 4, 0, 4.

Panels are on the exact-product grid of tests/test_gpu_topk_scores.py (every product and sum exact in float64, and every
value exact in float32), so the plain loop is the chain.
"""
import numpy as np
import pytest

import rank_entries_ref as RR
import topk_scores_ref as R

pytestmark = pytest.mark.gpu

ROWS, ITEMS, N_TOP = 5, 129, 4
USERS = np.array([4, 0, 4])
SPLITS = (None, 1, 2, 3)


def _csr(cols):
    from csr_amd import CSR
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    ci = np.concatenate([np.asarray(c, np.int32) for c in cols]).astype(np.int32)
    return CSR(ROWS, ITEMS, len(ci), rp, ci, None)


def _gather(mat, users):
    rp = np.concatenate([[0], np.cumsum(np.diff(mat.rowptrs)[users])]).astype(np.int64)
    ci = np.concatenate([mat.colinds[mat.rowptrs[u]:mat.rowptrs[u + 1]] for u in users]).astype(np.int32)
    return rp, ci


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope='module', params=[(4, np.float64), (5, np.float64), (4, np.float32), (5, np.float32)],
                ids=['k4-f64', 'k5-f64', 'k4-f32', 'k5-f32'])
def case(request):
    "panels (U strided), the two patterns, and the restatements on the gathered rows -- with `seen` and without -- once"
    k, dtype = request.param
    rng = np.random.default_rng(129 + k)
    wide_u = (rng.integers(-512, 512, (ROWS, k + 3)) / 64.0).astype(dtype)
    U = wide_u[:, :k]                                   # ldu = k + 3: rows 4 and 0 lie (k + 3) elements apart per row
    V = (rng.integers(-512, 512, (ITEMS, k)) / 64.0).astype(dtype)
    assert U.strides[0] == (k + 3) * U.itemsize and not U.flags['C_CONTIGUOUS']
    S = R.scores_plain(U, V)
    # `seen` is canonical, reaches every range of 3 splits -- [0, 64), [64, 128), [128, 129) -- and holds the best item of
    # row 4 and the second best of row 0, so that leaving it out changes both lists
    best = R.select(S, None, None, 2)[0]
    seen = _csr([sorted({int(best[0][1]), 0, 5, 63, 64, 128}), [], [1], [128], sorted({int(best[4][0]), 2, 64, 127, 128})])
    # `test` need not be sorted; rows 0 and 4 hold items of every range, seen and unseen
    test = _csr([[128, 3, 70], [7], [], [1, 2], [127, 128, 0, 65]])
    want = {}
    for with_seen in (True, False):
        srp, sci = _gather(seen, USERS) if with_seen else (None, None)
        trp, tci = _gather(test, USERS)
        want[with_seen] = (R.select(S[USERS], srp, sci, N_TOP), RR.ranks(S[USERS], srp, sci, trp, tci), RR.entry_scores(S[USERS], trp, tci))
    assert not np.array_equal(want[True][0][0], want[False][0][0]) and not np.array_equal(want[True][1], want[False][1])
    return U, V, seen, test, want


def test_strided_u_and_a_list_with_a_repeat_through_the_host_forms(case):
    from csr_amd.kernels import hip as K, releasing
    U, V, seen, test, want = case
    with releasing(K.to_handle(seen), K) as s, releasing(K.to_handle(test), K) as t:
        for with_seen in (True, False):
            sh = s if with_seen else None
            (w_items, w_scores, w_counts), w_ranks, w_entry = want[with_seen]
            # the range entries over all five rows, picked at the listed rows
            r_items, r_scores, r_counts = K.topk_scores(sh, U, V, N_TOP, None, (0, ROWS))
            r_ranks, r_entry = K.rank_entries(sh, t, U, V, (0, ROWS))
            pick = np.concatenate([np.arange(test.rowptrs[u], test.rowptrs[u + 1]) for u in USERS])
            for sp in SPLITS:
                what = (with_seen, sp)
                items, scores, counts = K.topk_scores_for(sh, USERS, U, V, N_TOP, None, sp)
                assert np.array_equal(items, w_items) and np.array_equal(counts, w_counts), what
                assert np.array_equal(_bits(scores), _bits(w_scores)), what
                assert np.array_equal(items, r_items[USERS]) and np.array_equal(counts, r_counts[USERS]), what
                assert np.array_equal(_bits(scores), _bits(r_scores[USERS])), what
                ranks, entry = K.rank_entries_for(sh, t, USERS, U, V, sp)
                assert np.array_equal(ranks, w_ranks) and np.array_equal(_bits(entry), _bits(w_entry)), what
                assert np.array_equal(ranks, r_ranks[pick]) and np.array_equal(_bits(entry), _bits(r_entry[pick])), what
    # both occurrences of row 4 got the same outputs, and they differ from row 0's: the list order reached the kernel
    assert np.array_equal(items[0], items[2]) and not np.array_equal(items[0], items[1])
