"""Stand-in backend for the host tests of `epilogos --groupings`: the oracle-backed sessions of tests/fake_backend.py plus the
calls a run over resident matrices makes -- stage (the "upload": counted, the matrix is a host array), add_device(columns=),
add_columns and close -- with the columns cut on the host.  Tests only."""
import numpy as np

from tests import fake_backend as fb


class _Resident:
    closed = False

    def stage(self, arr, N, ticket):
        self.n_uploads += 1
        return np.ascontiguousarray(arr[:, :N])

    def close(self):
        self.parts, self.counts, self.q, self.closed = [], None, None, True
        self.be.closed_sessions += 1


class _SingleSession(_Resident, fb._HostSingleSession):
    def add_device(self, X, N, columns=None):
        assert not self.closed
        x = X[:, :N] if columns is None else X[:, np.asarray(columns, dtype=np.int64)]
        return fb._HostSingleSession.add_part(self, x, x.shape[1], None)

    def add_part(self, arr, N, ticket, columns=None):
        return self.add_device(self.stage(arr, N, ticket), N, columns=columns)


class _PairedSession(_Resident, fb._HostPairedSession):
    def add_columns(self, X, N, colsA, colsB, row0):
        assert not self.closed
        a, b = np.asarray(colsA, dtype=np.int64), np.asarray(colsB, dtype=np.int64)
        return self.add_staged(X[:, a], a.size, X[:, b], b.size, row0)


class GroupingsBackend(fb.OracleBackend):
    name = "oracle-for-groupings-tests"

    def __init__(self):
        self.opened, self.closed_sessions = 0, 0

    def open_single(self, S, saliency):
        self.opened += 1
        return _SingleSession(self, S, saliency)

    def open_paired(self, S, saliency, quiescentState, groupSize, seed, draws=1):
        assert draws == 1
        self.opened += 1
        return _PairedSession(self, S, saliency, quiescentState, groupSize, seed)
