"""
Rules 4 and 11 of include/csrk.h -- into how many ranges csrk_topk_scores_for and csrk_rank_entries_for cut the items, and
the bytes of the former's workspace -- restated in plain Python from the library's limits, with the request grids the host
tests walk.  tests/test_topk_scores_for_host.py and tests/test_rank_entries_for_host.py compare the library with these,
tests/test_score_plan_host.py compares csr_amd/csrc/score_plan.h, as a stand-alone program, with the same text.
"""


def rule4(n_rows, n_items, n, splits, lim, tlim):
    "rule 4 and the workspace size, restated"
    s_max, w_small, w_large, slot, per = lim
    block, tile = tlim[2], tlim[3]
    T = -(-n_items // tile)
    if T == 0 or n_rows == 0:
        S = 1
    elif splits is not None:
        S = min(splits, T, s_max)
    else:
        W = w_small if n <= 32 else w_large
        S = max(1, min(-(-W // -(-n_rows // block)), T, s_max))
    nbytes = 0 if S == 1 else -(-(n_rows * S * (slot + per * (n - 1))) // 16) * 16
    return S, nbytes


def rule11(n_rows, n_items, splits, s_max, W, block, tile):
    "rule 11, restated"
    T = -(-n_items // tile)
    if T == 0 or n_rows == 0:
        return 1
    if splits is not None:
        return min(splits, T, s_max)
    return max(1, min(-(-W // -(-n_rows // block)), T, s_max))


RULE4_NS = (1, 2, 20, 32, 33, 128)


def rule4_grid(n, lim):
    "the (n_rows, n_items, splits) requests of the rule-4 test for lists of n"
    s_max = lim[0]
    W = lim[1] if n <= 32 else lim[2]
    for n_rows in (1, 64, 65, 1024, 64 * W, 64 * W - 64, 0):
        for n_items in (0, 1, 64, 65, 261, 64 * (s_max + 1), 2_000_000):
            for splits in (None, 1, 2, 3, 5, s_max, s_max + 1, 1000):
                yield n_rows, n_items, splits


def rule11_grid(s_max, W, tile):
    "the (n_rows, n_items, splits, T) requests of the rule-11 test"
    for n_rows in (0, 1, 64, 65, 64 * W, 64 * W + 1, 1024, 65536):
        for T in (0, 1, s_max, s_max + 1):
            for n_items in sorted({T * tile, max(T * tile - tile + 1, 0)} if T else {0}):
                for splits in (None, 1, 2, 3, 5, s_max, s_max + 1, T + 1, 1000):
                    yield n_rows, n_items, splits, T
