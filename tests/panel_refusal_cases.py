"""
Every refusal of the 14 C entries that take dense panels (include/csrk.h: csrk_spmm_dense, csrk_sddmm, csrk_gram_rows,
csrk_als_rows, csrk_solve_blocks, csrk_topk_scores, csrk_rank_entries, each with its _device form), as tables: what is changed
in a good request, the return code, and the EXACT text csrk_last_error() then holds.  The texts are literals, written down
from the sources before the entries' shared host steps moved into csrc/panel.h: a helper that words a refusal differently,
or an entry that checks in another order, fails here.  Rows with two faults at once pin the order.

The good request: a 3 x 4 matrix with rows of 2, 0 and 3 entries, k = 4 float64 panels, n_top = 2, n = 3 systems.
tests/test_panel_refusals.py runs what needs no handle (no GPU), tests/test_gpu_panel_refusals.py the rest.
"""
import numpy as np

INVALID, UNSUPPORTED = -1, -3
NAN, INF = float('nan'), float('inf')
NR, NC, NNZ, K, NTOP = 3, 4, 5, 4, 2
ROWPTRS, COLINDS = [0, 2, 2, 5], [0, 3, 0, 1, 2]
UNSORTED_COLINDS = [3, 0, 0, 1, 2]          # row 0 is not ascending
BAD_HANDLE, BAD_HANDLE_2 = 12345, 777
BAD_TEXT, BAD_TEXT_2 = 'invalid csrk handle 0x3039', 'invalid csrk handle 0x309'

PARAMS = {
    'csrk_spmm_dense': ('h', 'B', 'k', 'ldb', 'C', 'ldc'),
    'csrk_sddmm': ('h', 'U', 'ldu', 'V', 'ldv', 'k', 'pt', 'scale', 'out'),
    'csrk_gram_rows': ('h', 'rb', 're', 'V', 'ldv', 'k', 'pt', 'scale', 'base', 'out'),
    'csrk_als_rows': ('h', 'rb', 're', 'V', 'ldv', 'k', 'pt', 'scale', 'rhs', 'base', 'lam', 'out', 'ldo', 'info'),
    'csrk_solve_blocks': ('n', 'k', 'G', 'b', 'ldb', 'x', 'ldx', 'info'),
    'csrk_topk_scores': ('h', 'rb', 're', 'U', 'ldu', 'V', 'ldv', 'ni', 'k', 'pt', 'nt', 'ms', 'items', 'ldi', 'scores', 'lds', 'counts'),
    'csrk_rank_entries': ('seen', 'h', 'rb', 're', 'U', 'ldu', 'V', 'ldv', 'k', 'pt', 'ranks', 'scores'),
}

# the good request; '@name' is a handle the test supplies, '&name' the address of one of its buffers
GOOD = {
    'csrk_spmm_dense': dict(h='@mat', B='&V', k=K, ldb=K, C='&rows', ldc=K),
    'csrk_sddmm': dict(h='@mat', U='&U', ldu=K, V='&V', ldv=K, k=K, pt=2, scale=0, out='&nz'),
    'csrk_gram_rows': dict(h='@mat', rb=0, re=NR, V='&V', ldv=K, k=K, pt=2, scale=0, base=None, out='&gram'),
    'csrk_als_rows': dict(h='@mat', rb=0, re=NR, V='&V', ldv=K, k=K, pt=2, scale=0, rhs=1, base=None, lam=0.5, out='&rows', ldo=K,
                          info='&info'),
    'csrk_solve_blocks': dict(n=NR, k=K, G='&G', b='&U', ldb=K, x='&rows', ldx=K, info='&info'),
    'csrk_topk_scores': dict(h='@mat', rb=0, re=NR, U='&U', ldu=K, V='&V', ldv=K, ni=NC, k=K, pt=2, nt=NTOP, ms=-INF, items='&items',
                             ldi=NTOP, scores='&scores', lds=NTOP, counts='&counts'),
    'csrk_rank_entries': dict(seen='@mat', h='@mat', rb=0, re=NR, U='&U', ldu=K, V='&V', ldv=K, k=K, pt=2, ranks='&ranks', scores='&nz'),
}

PT7 = 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 7'
PT0 = 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 0'
K0 = 'k must be at least 1 (k=0)'
NOT_CANONICAL = ('seen is not canonical: row 0 is not strictly ascending in column (csrk_order_columns sorts, csrk_coalesce merges '
                 'repeats)')

# (what, forms, change, return code, text); forms: 'h' the host entry, 'd' the _device entry; '+name' = that buffer's
# address + 1 (misaligned).  A row that changes two things names both in `what`.
CASES = {
    'csrk_spmm_dense': [
        ('invalid handle', 'hd', dict(h=BAD_HANDLE), INVALID, BAD_TEXT),
        ('NULL B', 'hd', dict(B=None), INVALID, 'B or C is NULL'),
        ('NULL C', 'hd', dict(C=None), INVALID, 'B or C is NULL'),
        ('k < 0', 'h', dict(k=-1), INVALID, 'bad panel geometry'),
        ('ldb < k', 'h', dict(ldb=3), INVALID, 'bad panel geometry'),
        ('ldc < k', 'h', dict(ldc=3), INVALID, 'bad panel geometry'),
        ('k < 0', 'd', dict(k=-1), INVALID, 'bad panel geometry k=-1 ldb=4 ldc=4'),
        ('ldb < k', 'd', dict(ldb=3), INVALID, 'bad panel geometry k=4 ldb=3 ldc=4'),
        ('ldc < k', 'd', dict(ldc=3), INVALID, 'bad panel geometry k=4 ldb=4 ldc=3'),
        ('invalid handle + NULL B', 'hd', dict(h=BAD_HANDLE_2, B=None), INVALID, BAD_TEXT_2),
        ('NULL B + ldb < k', 'hd', dict(B=None, ldb=3), INVALID, 'B or C is NULL'),
        ('NULL C + k < 0', 'hd', dict(C=None, k=-1), INVALID, 'B or C is NULL'),
    ],
    'csrk_sddmm': [
        ('invalid handle', 'hd', dict(h=BAD_HANDLE), INVALID, BAD_TEXT),
        ('k = 0', 'hd', dict(k=0), INVALID, K0),
        ('k < 0', 'hd', dict(k=-2), INVALID, 'k must be at least 1 (k=-2)'),
        ('ldu < k', 'hd', dict(ldu=3), INVALID, 'bad panel geometry k=4 ldu=3 ldv=4'),
        ('ldv < k', 'hd', dict(ldv=3), INVALID, 'bad panel geometry k=4 ldu=4 ldv=3'),
        ('panel_type 7', 'hd', dict(pt=7), INVALID, PT7),
        ('panel_type none', 'hd', dict(pt=0), INVALID, PT0),
        ('scale 2', 'hd', dict(scale=2), INVALID, 'scale must be 0 or 1, not 2'),
        ('scale -1', 'hd', dict(scale=-1), INVALID, 'scale must be 0 or 1, not -1'),
        ('NULL U', 'hd', dict(U=None), INVALID, 'U, V or out is NULL'),
        ('NULL V', 'hd', dict(V=None), INVALID, 'U, V or out is NULL'),
        ('NULL out', 'hd', dict(out=None), INVALID, 'U, V or out is NULL'),
        ('misaligned U', 'd', dict(U='+U'), INVALID, 'U, V or out is not aligned to its element size'),
        ('misaligned out', 'd', dict(out='+nz'), INVALID, 'U, V or out is not aligned to its element size'),
        ('invalid handle + k = 0', 'hd', dict(h=BAD_HANDLE, k=0), INVALID, BAD_TEXT),
        ('k = 0 + panel_type 7', 'hd', dict(k=0, pt=7), INVALID, K0),
        ('ldv < k + scale 2', 'hd', dict(ldv=3, scale=2), INVALID, 'bad panel geometry k=4 ldu=4 ldv=3'),
        ('panel_type 7 + NULL U', 'hd', dict(pt=7, U=None), INVALID, PT7),
        ('scale 2 + NULL out', 'hd', dict(scale=2, out=None), INVALID, 'scale must be 0 or 1, not 2'),
    ],
    'csrk_gram_rows': [
        ('invalid handle', 'hd', dict(h=BAD_HANDLE), INVALID, BAD_TEXT),
        ('k = 0', 'hd', dict(k=0), INVALID, K0),
        ('k < 0', 'hd', dict(k=-1), INVALID, 'k must be at least 1 (k=-1)'),
        ('ldv < k', 'hd', dict(ldv=3), INVALID, 'bad panel geometry k=4 ldv=3'),
        ('panel_type 7', 'hd', dict(pt=7), INVALID, PT7),
        ('panel_type none', 'hd', dict(pt=0), INVALID, PT0),
        ('scale 2', 'hd', dict(scale=2), INVALID, 'scale must be 0 or 1, not 2'),
        ('row_begin < 0', 'hd', dict(rb=-1), INVALID, 'bad row range [-1, 3) of 3 rows'),
        ('row_end > nrows', 'hd', dict(re=4), INVALID, 'bad row range [0, 4) of 3 rows'),
        ('row_begin > row_end', 'hd', dict(rb=2, re=1), INVALID, 'bad row range [2, 1) of 3 rows'),
        ('k above the limit', 'hd', dict(k=129, ldv=129), UNSUPPORTED,
         'csrk_gram_rows: k=129 is above the largest supported k=128 (csrk_gram_limits)'),
        ('NULL V', 'hd', dict(V=None), INVALID, 'V or out is NULL'),
        ('NULL out', 'hd', dict(out=None), INVALID, 'V or out is NULL'),
        ('misaligned V', 'd', dict(V='+V'), INVALID, 'V, base or out is not aligned to its element size'),
        ('misaligned base', 'd', dict(base='+G'), INVALID, 'V, base or out is not aligned to its element size'),
        ('k = 0 + panel_type 7', 'hd', dict(k=0, pt=7), INVALID, K0),
        ('ldv < k + reversed rows', 'hd', dict(ldv=3, rb=2, re=1), INVALID, 'bad panel geometry k=4 ldv=3'),
        ('k above the limit + row_end > nrows', 'hd', dict(k=129, ldv=129, re=4), INVALID, 'bad row range [0, 4) of 3 rows'),
        ('scale 2 + row_begin < 0', 'hd', dict(scale=2, rb=-1), INVALID, 'scale must be 0 or 1, not 2'),
        ('panel_type 7 + scale 2', 'hd', dict(pt=7, scale=2), INVALID, PT7),
        ('k above the limit + NULL V', 'hd', dict(k=129, ldv=129, V=None), UNSUPPORTED,
         'csrk_gram_rows: k=129 is above the largest supported k=128 (csrk_gram_limits)'),
    ],
    'csrk_als_rows': [
        ('invalid handle', 'hd', dict(h=BAD_HANDLE), INVALID, BAD_TEXT),
        ('k = 0', 'hd', dict(k=0), INVALID, K0),
        ('ldv < k', 'hd', dict(ldv=3), INVALID, 'bad panel geometry k=4 ldv=3'),
        ('ldo < k', 'hd', dict(ldo=3), INVALID, 'bad output geometry k=4 ldo=3'),
        ('panel_type 7', 'hd', dict(pt=7), INVALID, PT7),
        ('scale 2', 'hd', dict(scale=2), INVALID, 'scale must be 0 or 1, not 2'),
        ('rhs_mode 5', 'hd', dict(rhs=5), INVALID, 'rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not 5'),
        ('rhs_mode -1', 'hd', dict(rhs=-1), INVALID, 'rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not -1'),
        ('row_begin < 0', 'hd', dict(rb=-1), INVALID, 'bad row range [-1, 3) of 3 rows'),
        ('row_end > nrows', 'hd', dict(re=4), INVALID, 'bad row range [0, 4) of 3 rows'),
        ('row_begin > row_end', 'hd', dict(rb=2, re=1), INVALID, 'bad row range [2, 1) of 3 rows'),
        ('k above the limit', 'hd', dict(k=129, ldv=129, ldo=129), UNSUPPORTED,
         'csrk_als_rows: k=129 is above the largest supported k=128 (csrk_als_limits)'),
        ('NULL V', 'hd', dict(V=None), INVALID, 'V or out is NULL'),
        ('NULL out', 'hd', dict(out=None), INVALID, 'V or out is NULL'),
        ('misaligned V', 'd', dict(V='+V'), INVALID, 'V, base, out or info is not aligned to its element size'),
        ('misaligned info', 'd', dict(info='+info'), INVALID, 'V, base, out or info is not aligned to its element size'),
        ('k = 0 + panel_type 7', 'hd', dict(k=0, pt=7), INVALID, K0),
        ('ldv < k + ldo < k', 'hd', dict(ldv=3, ldo=3), INVALID, 'bad panel geometry k=4 ldv=3'),
        ('ldv < k + reversed rows', 'hd', dict(ldv=3, rb=2, re=1), INVALID, 'bad panel geometry k=4 ldv=3'),
        ('ldo < k + panel_type 7', 'hd', dict(ldo=3, pt=7), INVALID, 'bad output geometry k=4 ldo=3'),
        ('scale 2 + rhs_mode 5', 'hd', dict(scale=2, rhs=5), INVALID, 'scale must be 0 or 1, not 2'),
        ('rhs_mode 5 + row_end > nrows', 'hd', dict(rhs=5, re=4), INVALID, 'rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not 5'),
        ('k above the limit + row_end > nrows', 'hd', dict(k=129, ldv=129, ldo=129, re=4), INVALID, 'bad row range [0, 4) of 3 rows'),
    ],
    'csrk_solve_blocks': [
        ('n < 0', 'hd', dict(n=-1), INVALID, 'n must not be negative (n=-1)'),
        ('k = 0', 'hd', dict(k=0), INVALID, K0),
        ('ldb < k', 'hd', dict(ldb=3), INVALID, 'bad geometry k=4 ldb=3 ldx=4'),
        ('ldx < k', 'hd', dict(ldx=3), INVALID, 'bad geometry k=4 ldb=4 ldx=3'),
        ('k above the limit', 'hd', dict(k=129, ldb=129, ldx=129), UNSUPPORTED,
         'csrk_solve_blocks: k=129 is above the largest supported k=128 (csrk_als_limits)'),
        ('NULL G', 'hd', dict(G=None), INVALID, 'G, b or x is NULL'),
        ('NULL b', 'hd', dict(b=None), INVALID, 'G, b or x is NULL'),
        ('NULL x', 'hd', dict(x=None), INVALID, 'G, b or x is NULL'),
        ('misaligned G', 'd', dict(G='+G'), INVALID, 'G, b, x or info is not aligned to its element size'),
        ('misaligned info', 'd', dict(info='+info'), INVALID, 'G, b, x or info is not aligned to its element size'),
        ('more systems than a launch takes', 'd', dict(n=2 ** 36), INVALID, 'n=68719476736 systems are more than one launch takes'),
        ('n < 0 + k = 0', 'hd', dict(n=-1, k=0), INVALID, 'n must not be negative (n=-1)'),
        ('k = 0 + ldb < k', 'hd', dict(k=0, ldb=-1), INVALID, K0),
        ('ldb < k + k above the limit', 'hd', dict(k=129, ldb=3, ldx=129), INVALID, 'bad geometry k=129 ldb=3 ldx=129'),
        ('k above the limit + NULL G', 'hd', dict(k=129, ldb=129, ldx=129, G=None), UNSUPPORTED,
         'csrk_solve_blocks: k=129 is above the largest supported k=128 (csrk_als_limits)'),
    ],
    # seen = 0: needs no handle
    'csrk_topk_scores': [
        ('k = 0', 'hd', dict(k=0), INVALID, 'topk_scores: ' + K0),
        ('n_top = 0', 'hd', dict(nt=0), INVALID, 'topk_scores: n_top must be at least 1 (n_top=0)'),
        ('n_items < 0', 'hd', dict(ni=-1), INVALID, 'topk_scores: n_items must not be negative (n_items=-1)'),
        ('ldu < k', 'hd', dict(ldu=3), INVALID, 'topk_scores: bad panel geometry k=4 ldu=3 ldv=4'),
        ('ldv < k', 'hd', dict(ldv=3), INVALID, 'topk_scores: bad panel geometry k=4 ldu=4 ldv=3'),
        ('ldi < n_top', 'hd', dict(ldi=1), INVALID, 'topk_scores: bad output geometry n_top=2 ldi=1 lds=2'),
        ('lds < n_top', 'hd', dict(lds=1), INVALID, 'topk_scores: bad output geometry n_top=2 ldi=2 lds=1'),
        ('panel_type 7', 'hd', dict(pt=7), INVALID, 'topk_scores: ' + PT7),
        ('panel_type none', 'hd', dict(pt=0), INVALID, 'topk_scores: ' + PT0),
        ('NaN min_score', 'hd', dict(ms=NAN), INVALID, 'topk_scores: min_score is NaN'),
        ('row_begin < 0', 'hd', dict(rb=-1), INVALID, 'topk_scores: bad row range [-1, 3)'),
        ('row_begin > row_end', 'hd', dict(rb=3, re=2), INVALID, 'topk_scores: bad row range [3, 2)'),
        ('k above the limit', 'hd', dict(k=1025, ldu=1025, ldv=1025), UNSUPPORTED,
         'csrk_topk_scores: k=1025 is above the largest supported k=1024 (csrk_topk_scores_limits)'),
        ('n_top above the limit', 'hd', dict(nt=129, ldi=129, lds=129), UNSUPPORTED,
         'csrk_topk_scores: n_top=129 is above the largest supported n_top=128 (csrk_topk_scores_limits)'),
        ('NULL items', 'hd', dict(items=None), INVALID, 'topk_scores: items or scores is NULL'),
        ('NULL scores', 'hd', dict(scores=None), INVALID, 'topk_scores: items or scores is NULL'),
        ('NULL U', 'hd', dict(U=None), INVALID, 'topk_scores: U is NULL'),
        ('NULL V', 'hd', dict(V=None), INVALID, 'topk_scores: V is NULL'),
        ('misaligned U', 'd', dict(U='+U'), INVALID, 'topk_scores: U, V, items, scores or counts is not aligned to its element size'),
        ('misaligned counts', 'd', dict(counts='+counts'), INVALID,
         'topk_scores: U, V, items, scores or counts is not aligned to its element size'),
        ('k = 0 + panel_type 7', 'hd', dict(k=0, pt=7), INVALID, 'topk_scores: ' + K0),
        ('ldv < k + reversed rows', 'hd', dict(ldv=3, rb=2, re=1), INVALID, 'topk_scores: bad panel geometry k=4 ldu=4 ldv=3'),
        ('k above the limit + n_top = 0', 'hd', dict(k=1025, ldu=1025, ldv=1025, nt=0), INVALID,
         'topk_scores: n_top must be at least 1 (n_top=0)'),
        ('n_top = 0 + n_items < 0', 'hd', dict(nt=0, ni=-1), INVALID, 'topk_scores: n_top must be at least 1 (n_top=0)'),
        ('ldi < n_top + panel_type 7', 'hd', dict(ldi=1, pt=7), INVALID, 'topk_scores: bad output geometry n_top=2 ldi=1 lds=2'),
        ('NaN min_score + row_begin < 0', 'hd', dict(ms=NAN, rb=-1), INVALID, 'topk_scores: min_score is NaN'),
        ('k above the limit + reversed rows', 'hd', dict(k=1025, ldu=1025, ldv=1025, rb=2, re=1), INVALID,
         'topk_scores: bad row range [2, 1)'),
        ('k and n_top above the limits', 'hd', dict(k=1025, ldu=1025, ldv=1025, nt=129, ldi=129, lds=129), UNSUPPORTED,
         'csrk_topk_scores: k=1025 is above the largest supported k=1024 (csrk_topk_scores_limits)'),
        ('k above the limit + NULL items', 'hd', dict(k=1025, ldu=1025, ldv=1025, items=None), UNSUPPORTED,
         'csrk_topk_scores: k=1025 is above the largest supported k=1024 (csrk_topk_scores_limits)'),
        ('NULL items + NULL U', 'hd', dict(items=None, U=None), INVALID, 'topk_scores: items or scores is NULL'),
        ('NULL U + NULL V', 'hd', dict(U=None, V=None), INVALID, 'topk_scores: U is NULL'),
    ],
    # ... and what a seen handle adds (the rows above hold with one as well)
    'csrk_topk_scores with seen': [
        ('invalid handle', 'hd', dict(h=BAD_HANDLE), INVALID, BAD_TEXT),
        ('invalid handle + k = 0', 'hd', dict(h=BAD_HANDLE_2, k=0), INVALID, BAD_TEXT_2),
        ('row_end > nrows', 'hd', dict(re=4), INVALID, 'topk_scores: bad row range [0, 4) of 3 rows'),
        ('n_items is not ncols', 'hd', dict(ni=5), INVALID, 'topk_scores: n_items=5 but seen has 4 columns'),
        ('seen is not canonical', 'hd', dict(h='@unsorted'), INVALID, 'topk_scores: ' + NOT_CANONICAL),
        ('k above the limit + row_end > nrows', 'hd', dict(k=1025, ldu=1025, ldv=1025, re=4), INVALID,
         'topk_scores: bad row range [0, 4) of 3 rows'),
        ('row_end > nrows + n_items is not ncols', 'hd', dict(re=4, ni=5), INVALID, 'topk_scores: bad row range [0, 4) of 3 rows'),
        ('n_items is not ncols + not canonical', 'hd', dict(h='@unsorted', ni=5), INVALID, 'topk_scores: n_items=5 but seen has 4 columns'),
        ('not canonical + k above the limit', 'hd', dict(h='@unsorted', k=1025, ldu=1025, ldv=1025), INVALID,
         'topk_scores: ' + NOT_CANONICAL),
        ('NaN min_score + row_end > nrows', 'hd', dict(ms=NAN, re=4), INVALID, 'topk_scores: min_score is NaN'),
    ],
    # the scalars are looked at before the handles: these need none (the test passes two invalid ones where it has none)
    'csrk_rank_entries': [
        ('k = 0', 'hd', dict(k=0), INVALID, 'rank_entries: ' + K0),
        ('ldu < k', 'hd', dict(ldu=3), INVALID, 'rank_entries: bad panel geometry k=4 ldu=3 ldv=4'),
        ('ldv < k', 'hd', dict(ldv=3), INVALID, 'rank_entries: bad panel geometry k=4 ldu=4 ldv=3'),
        ('panel_type 7', 'hd', dict(pt=7), INVALID, 'rank_entries: ' + PT7),
        ('panel_type none', 'hd', dict(pt=0), INVALID, 'rank_entries: ' + PT0),
        ('row_begin < 0', 'hd', dict(rb=-1), INVALID, 'rank_entries: bad row range [-1, 3)'),
        ('row_begin > row_end', 'hd', dict(rb=3, re=2), INVALID, 'rank_entries: bad row range [3, 2)'),
        ('k above the limit', 'hd', dict(k=1025, ldu=1025, ldv=1025), UNSUPPORTED,
         'csrk_rank_entries: k=1025 is above the largest supported k=1024 (csrk_rank_entries_limits)'),
        ('invalid seen', 'hd', dict(seen=BAD_HANDLE), INVALID, BAD_TEXT),
        ('invalid test', 'hd', dict(h=BAD_HANDLE_2), INVALID, BAD_TEXT_2),
        ('k = 0 + panel_type 7', 'hd', dict(k=0, pt=7), INVALID, 'rank_entries: ' + K0),
        ('ldv < k + reversed rows', 'hd', dict(ldv=3, rb=2, re=1), INVALID, 'rank_entries: bad panel geometry k=4 ldu=4 ldv=3'),
        ('k above the limit + row_end > nrows', 'hd', dict(k=1025, ldu=1025, ldv=1025, re=4), UNSUPPORTED,
         'csrk_rank_entries: k=1025 is above the largest supported k=1024 (csrk_rank_entries_limits)'),
        ('panel_type 7 + invalid test', 'hd', dict(pt=7, h=BAD_HANDLE), INVALID, 'rank_entries: ' + PT7),
        ('k above the limit + invalid seen', 'hd', dict(k=1025, ldu=1025, ldv=1025, seen=BAD_HANDLE), UNSUPPORTED,
         'csrk_rank_entries: k=1025 is above the largest supported k=1024 (csrk_rank_entries_limits)'),
        ('invalid seen + invalid test', 'hd', dict(seen=BAD_HANDLE, h=BAD_HANDLE_2), INVALID, BAD_TEXT),
    ],
    'csrk_rank_entries with handles': [
        ('row_end > nrows', 'hd', dict(re=4), INVALID, 'rank_entries: bad row range [0, 4) of 3 rows'),
        ('seen of another shape', 'hd', dict(seen='@wide'), INVALID, 'rank_entries: seen is 3 x 5 but test is 3 x 4'),
        ('seen is not canonical', 'hd', dict(seen='@unsorted'), INVALID, 'rank_entries: ' + NOT_CANONICAL),
        ('NULL ranks', 'hd', dict(ranks=None), INVALID, 'rank_entries: ranks is NULL'),
        ('NULL U', 'hd', dict(U=None), INVALID, 'rank_entries: U or V is NULL'),
        ('NULL V', 'hd', dict(V=None), INVALID, 'rank_entries: U or V is NULL'),
        ('misaligned U', 'hd', dict(U='+U'), INVALID, 'rank_entries: U, V, ranks or scores is not aligned to its element size'),
        ('misaligned ranks', 'hd', dict(ranks='+ranks'), INVALID, 'rank_entries: U, V, ranks or scores is not aligned to its element size'),
        ('row_end > nrows + seen of another shape', 'hd', dict(re=4, seen='@wide'), INVALID, 'rank_entries: bad row range [0, 4) of 3 rows'),
        ('seen of another shape + NULL ranks', 'hd', dict(seen='@wide', ranks=None), INVALID, 'rank_entries: seen is 3 x 5 but test is 3 x 4'),
        ('not canonical + NULL U', 'hd', dict(seen='@unsorted', U=None), INVALID, 'rank_entries: ' + NOT_CANONICAL),
        ('NULL ranks + NULL U', 'hd', dict(ranks=None, U=None), INVALID, 'rank_entries: ranks is NULL'),
    ],
}

NO_HANDLE = ('csrk_solve_blocks', 'csrk_topk_scores', 'csrk_rank_entries')          # tables that run without a GPU


class Buffers:
    "the good request's arrays -- NumPy, or torch tensors on the card for the _device entries -- outputs filled with 7"
    INPUTS = dict(U=((NR, K), 'f8'), V=((NC, K), 'f8'), G=((NR, K, K), 'f8'))
    OUTPUTS = dict(rows=((NR, K), 'f8'), nz=((NNZ,), 'f8'), gram=((NR, K, K), 'f8'), info=((NR,), 'i4'), items=((NR, NTOP), 'i4'),
                   scores=((NR, NTOP), 'f8'), counts=((NR,), 'i4'), ranks=((NNZ,), 'i4'))

    def __init__(self, on_card):
        self.a = {}
        for name, (shape, dt) in {**self.INPUTS, **self.OUTPUTS}.items():
            a = np.full(shape, 7, dt)
            if name == 'G':
                a[:] = np.eye(K)
            if on_card:
                import torch
                a = torch.from_numpy(a).cuda()
            self.a[name] = a
        self.on_card = on_card

    def address(self, name):
        return self.a[name].data_ptr() if self.on_card else self.a[name].ctypes.data

    def outputs_untouched(self):
        if self.on_card:
            import torch
            torch.cuda.synchronize()
        return all(bool((self.a[name] == 7).all()) for name in self.OUTPUTS)


def arguments(entry, change, bufs, handles):
    "the argument tuple of `entry` (a key of PARAMS) for the good request with `change` applied; stream NULL is the caller's to add"
    a = dict(GOOD[entry], **change)

    def value(v):
        if isinstance(v, str) and v[0] == '@':
            return handles[v[1:]]
        if isinstance(v, str) and v[0] == '&':
            return bufs.address(v[1:])
        if isinstance(v, str) and v[0] == '+':
            return bufs.address(v[1:]) + 1
        return v
    return tuple(value(a[p]) for p in PARAMS[entry])


def run_table(lib, table, entry, bufs_host, bufs_device, handles, only=''):
    """
    every row of CASES[table] (whose `what` holds `only`) through `entry` and its _device form: the code, the exact text, and
    at the end nothing written
    """
    for what, forms, change, rc, text in CASES[table]:
        if only not in what:
            continue
        for form in forms:
            fn = getattr(lib, entry + ('_device' if form == 'd' else ''))
            bufs = bufs_device if form == 'd' else bufs_host
            args = arguments(entry, change, bufs, handles) + ((None,) if form == 'd' else ())
            got = fn(*args)
            assert got == rc, (fn.__name__, what, got, lib.csrk_last_error())
            assert lib.csrk_last_error().decode() == text, (fn.__name__, what, lib.csrk_last_error())
    assert bufs_host.outputs_untouched() and bufs_device.outputs_untouched(), (entry, table)
