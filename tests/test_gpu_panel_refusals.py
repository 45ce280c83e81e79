"""
The refusals of the 14 dense-panel C entries on the card, word for word (tests/panel_refusal_cases.py has the tables): each
row through the host and the _device entry of a 3 x 4 matrix with rows of 2, 0 and 3 entries, k = 4 -- the return code, the
exact csrk_last_error() text, and nothing written into the sentinel-filled outputs.  The _device entries get buffers on the
card, so that a refusal that went missing would compute instead of faulting.
"""
import numpy as np
import pytest

import panel_refusal_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def handles():
    from csr_amd import CSR
    from csr_amd.kernels import hip as K

    def csr(nc, ci):
        return CSR(P.NR, nc, P.NNZ, np.array(P.ROWPTRS, np.int32), np.array(ci, np.int32), np.ones(P.NNZ), _cast=False)
    hs = {'mat': K.to_handle(csr(P.NC, P.COLINDS)), 'wide': K.to_handle(csr(P.NC + 1, P.COLINDS)),
          'unsorted': K.to_handle(csr(P.NC, P.UNSORTED_COLINDS))}
    yield {name: h.H for name, h in hs.items()}
    for h in hs.values():
        K.release_handle(h)


@pytest.mark.parametrize('table', sorted(P.CASES))
def test_refusals_word_for_word(table, handles):
    from csr_amd._lib import lib
    host, dev = P.Buffers(False), P.Buffers(True)
    P.run_table(lib, table, table.split(' ')[0], host, dev, handles)
    if table == 'csrk_topk_scores':          # the same rows with nothing seen
        P.run_table(lib, table, 'csrk_topk_scores', host, dev, {'mat': 0})


def test_the_handles_still_compute(handles):
    "after every refusal above (the fixture is the module's): the good request of each host entry is answered"
    from csr_amd._lib import lib
    host = P.Buffers(False)
    for entry in P.PARAMS:
        assert getattr(lib, entry)(*P.arguments(entry, {}, host, handles)) == 0, (entry, lib.csrk_last_error())
    assert not host.outputs_untouched()
