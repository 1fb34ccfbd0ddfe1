"""fv_set_model_sparse without a GPU: the symbol is exported and listed, dense_to_csr round-trips, make_model_csr emits
well-formed CSR of the requested shape."""
import numpy as np

from flash_viterbi_amd import decoder
from flash_viterbi_amd.generate_data import data_script


def csr_to_dense(indptr, indices, data, K):
    A = np.zeros((K, K), dtype=np.float32)
    A[np.repeat(np.arange(K), np.diff(indptr)), indices] = data
    return A


def test_library_exports_fv_set_model_sparse():
    lib = decoder.load_library()
    assert hasattr(lib, "fv_set_model_sparse")
    assert "fv_set_model_sparse" in decoder.EXPORTS
    assert decoder.KERNEL_SPARSE_CSR == 7
    assert hasattr(decoder.FlashViterbi, "set_model_sparse")


def test_dense_to_csr_round_trips():
    rs = np.random.RandomState(3)
    K = 37
    A = (rs.uniform(0.1, 1.0, (K, K)) * (rs.uniform(0, 1, (K, K)) < 0.2)).astype(np.float32)
    A[5] = 0.0                         # empty rows (first, middle, last) and empty columns
    A[0] = 0.0
    A[K - 1] = 0.0
    A[:, 7] = 0.0
    A[:, 0] = 0.0
    A[:, K - 1] = 0.0
    A[3, 4] = 0.0                      # "stored zeros" of the dense form: absent in CSR
    indptr, indices, data = decoder.dense_to_csr(A)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.shape == (K + 1,) and indptr[0] == 0 and indptr[-1] == indices.size == data.size == np.count_nonzero(A)
    assert (np.diff(indptr) >= 0).all() and indptr[6] == indptr[5] and indptr[1] == 0 and indptr[K] == indptr[K - 1]
    for k in range(K):
        cols = indices[indptr[k]:indptr[k + 1]]
        assert (np.diff(cols) > 0).all() and ((cols >= 0) & (cols < K)).all()
    assert (data != 0).all()
    assert np.array_equal(csr_to_dense(indptr, indices, data, K), A)
    # all-zero and full matrices
    z = decoder.dense_to_csr(np.zeros((4, 4), np.float32))
    assert z[0].tolist() == [0, 0, 0, 0, 0] and z[1].size == 0 and z[2].size == 0
    f = decoder.dense_to_csr(np.full((3, 3), 0.25, np.float32))
    assert f[0].tolist() == [0, 3, 6, 9] and f[1].tolist() == [0, 1, 2] * 3


def test_make_model_csr_is_well_formed():
    for K, M, d in ((500, 6, 12), (300, 4, 0.05), (64, 3, 1)):
        indptr, indices, data, B, Pi = data_script.make_model_csr(K, M, 11, d)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
        assert indptr[0] == 0 and indptr[-1] == indices.size == data.size and B.shape == (K, M) and Pi.shape == (K,)
        deg = np.diff(indptr)
        assert (deg >= 1).all()                               # every state has a successor
        mean = d if d >= 1 else d * K
        assert abs(deg.mean() - max(mean, 1)) < 0.25 * max(mean, 1) + 0.5
        for k in range(K):
            cols = indices[indptr[k]:indptr[k + 1]]
            assert (np.diff(cols) > 0).all() and cols[0] >= 0 and cols[-1] < K
        assert ((data > 0) & (data <= 1)).all()
        sums = np.add.reduceat(data.astype(np.float64), indptr[:-1])
        assert np.allclose(sums, 1.0, atol=1e-5)
        again = data_script.make_model_csr(K, M, 11, d)
        assert all(np.array_equal(a, b) for a, b in zip((indptr, indices, data, B, Pi), again))
