"""GPU: stats()["device_bytes"] over the life of one context — every way of setting a model or emission scores and
every decode entry point, in a fixed order.

Buffers only grow and every size is a sum of n * sizeof, so the sequence is deterministic.  The expected values are
what commit 6ffe9ef ("Add FV_KERNEL_CSR_F64") reported for this script on an MI355X, the last commit whose accounting
was a hand-written sum over the context's buffers; they pin the enumeration of the buffers that replaced it (a buffer
left out of it, or a table a model setter forgets to drop, shows here).  A second context that runs the same steps
must report the same list: nothing is shared or leaked between contexts."""
import numpy as np
import pytest

import modelgen
from flash_viterbi_amd import decoder

pytestmark = pytest.mark.gpu

K, M, T, N, BEAM = 64, 8, 16, 2, 4
SPEC = dict(kind="data_script", K=K, M=M, T=T, prob=0.3, seed=5)
LENGTHS = (16, 9, 5)

# (step, device_bytes after it) from that commit.  The device statistics block has since grown by one 64-bit word (the
# back-tracks' retry counter, fv_stats.bt_restarts): 8 bytes in the counters buffer and 8 in the result block that carries
# them to the host, in every figure after the first decode has allocated the two.
BT_WORD = 16
EXPECTED = [
    ("set_model", 80416),
    ("decode_full", 86592 + BT_WORD),
    ("decode_beam", 219480 + BT_WORD),
    ("decode_full_batch", 224824 + BT_WORD),
    ("decode_beam_batch", 298160 + BT_WORD),
    ("set_emissions", 310464 + BT_WORD),
    ("decode_full on emissions", 310464 + BT_WORD),
    ("set_model_sparse", 231084 + BT_WORD),
    ("decode_full on the sparse model", 231084 + BT_WORD),
    ("set_model again", 261312 + BT_WORD),
    ("decode_full again", 261312 + BT_WORD),
]


def _steps(fv, A, B, Pi, ob):
    seqs = [ob[:n] for n in LENGTHS]
    emis = np.log(np.random.RandomState(11).uniform(0.05, 1.0, (T, K))).astype(np.float32)
    got = []

    def record(step):
        got.append((step, fv.stats()["device_bytes"]))

    fv.set_model(A, B, Pi)
    record("set_model")
    fv.decode_full(ob, N)
    record("decode_full")
    fv.decode_beam(ob, N, BEAM)
    record("decode_beam")
    fv.decode_full_batch(seqs, N)
    record("decode_full_batch")
    fv.decode_beam_batch(seqs, N, BEAM)
    record("decode_beam_batch")
    fv.set_emissions(emis)
    record("set_emissions")
    fv.decode_full(None, N, T=T)
    record("decode_full on emissions")
    fv.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
    record("set_model_sparse")
    fv.decode_full(ob, N)
    record("decode_full on the sparse model")
    fv.set_model(A, B, Pi)
    record("set_model again")
    fv.decode_full(ob, N)
    record("decode_full again")
    return got


def test_device_bytes_of_every_entry_point_in_turn():
    A, B, Pi, ob = modelgen.model32(SPEC)
    first, second = decoder.FlashViterbi(0), decoder.FlashViterbi(0)
    try:
        got = _steps(first, A, B, Pi, ob)
        print("device_bytes:", got)
        assert got == EXPECTED
        assert _steps(second, A, B, Pi, ob) == EXPECTED
    finally:
        first.close()
        second.close()
