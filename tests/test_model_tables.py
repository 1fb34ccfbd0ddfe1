"""The host model builders of fv_set_model and fv_set_model_sparse (csrc/fv_model.cpp) without a GPU, through
fv_test_model_digest: every host table as an FNV-1a digest, the window / scale / density parameters, and the refusals with
their sentences.

EXPECTED was recorded from the builders as they stood before they were moved into fv_model.cpp and given one Q16 rule
and one value check (the same hook applied to an untouched copy of them); every assertion is an equality, so the builders
still make the same bytes.  The shapes sit where a layout rule changes: K = 5 one partial tile, 16 / 17 the tile edge,
37 three tiles with empty rows and columns first, middle and last, 130 (nrows = 160), 300 (the row loops go multi-threaded
at 256 rows); densities 1.0 and about 0.2; one model with entries in (1, 50]; one all-zero A (no finite log: the Q16 step
falls back to 1).

That a dense-set and a CSR-set model of one matrix DECODE alike is asserted on the GPU by tests/test_gpu_sparse.py; here
the two builders are held to the same qscale, windowq, density, any_big and log B / log Pi bytes on the CPU."""
import numpy as np
import pytest

from flash_viterbi_amd import decoder
from modelgen import plain_model as make_model

ERR_ARG = decoder.ERR_ARG
SHARED_DIGESTS = ("b64", "b32", "pi64")
SHARED_PARAMS = ("qscale", "windowq", "density", "any_big")


def hollow(A):
    """rows and columns 0, K // 2 and K - 1 emptied"""
    A = A.copy()
    for k in (0, A.shape[0] // 2, A.shape[0] - 1):
        A[k, :] = 0
        A[:, k] = 0
    return A


def csr_with_stored_zeros(A, seed):
    """CSR of A that also stores about a tenth of its zero entries, as explicit zeros"""
    rng = np.random.default_rng(seed)
    stored = (A != 0) | (rng.random(A.shape, dtype=np.float32) < np.float32(0.1))
    rows, cols = np.nonzero(stored)
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=indptr[1:])
    return indptr, cols.astype(np.int32), A[rows, cols]


def models():
    out = {}
    for K, M in ((5, 3), (16, 4), (17, 3), (37, 4), (130, 3), (300, 4)):
        for density in (1.0, 0.2):
            A, B, Pi = make_model(K, M, density, seed=1000 * K + int(10 * density))
            if K == 37:
                A = hollow(A)
            out["K%d_d%02d" % (K, int(10 * density))] = (A, B, Pi)
    out["K37_big"] = make_model(37, 3, 0.5, seed=7, scale=32.0)           # entries up to 32
    out["K17_zero"] = make_model(17, 3, 1.0, seed=8, zero_a=True)
    return out


MODELS = models()


def forms(name):
    """the digests of model `name`: its dense form, its dense_to_csr form and (K = 37) a CSR form with stored zeros"""
    A, B, Pi = MODELS[name]
    out = {"dense": decoder.test_model_digest(A, B, Pi), "csr": decoder.test_model_digest(decoder.dense_to_csr(A), B, Pi)}
    if name.startswith("K37_d"):
        out["csr_zeros"] = decoder.test_model_digest(csr_with_stored_zeros(A, seed=37), B, Pi)
    return out


# name -> form -> (digests in the order of decoder.MODEL_DIGESTS_DENSE / _CSR, params in the order of decoder.MODEL_PARAMS as
# float.hex()): recorded, see the module docstring
EXPECTED = {
    "K130_d02": {
        "dense": ((0xa6cfe04b20f3ba46, 0xbadf6762f160d144, 0x036810fcd19ba2eb, 0x52beef1606b1b80a, 0xe77e270913eba576, 0xb5b3ac7a55d1d373, 0x9beaa8557170f446, 0xa247eec1314b1509, 0xf1aedd2170af7704, 0xd04d11266ea97749),
                  ("0x1.504f1a0000000p-8", "0x1.5304400000000p-13", "-0x1.530f2a0000000p-13", "0x1.9f89b997a93b9p-3", "0x0.0p+0")),
        "csr": ((0xaf4b5dd18415edcd, 0x37ff3b14440047fa, 0x57b0e473a4fcfed2, 0xcbb10bffed1b1523, 0x9beaa8557170f446, 0x9b00c4897474a677, 0xa247eec1314b1509, 0xf1aedd2170af7704, 0xd04d11266ea97749),
                  ("0x0.0p+0", "0x1.5304400000000p-13", "-0x1.530f2a0000000p-13", "0x1.9f89b997a93b9p-3", "0x0.0p+0")),
    },
    "K130_d10": {
        "dense": ((0x91c1d0896a789ac3, 0x32faa9815095ff01, 0x9d738e1a68fac083, 0x74187cfbc20d8d77, 0xedb594769d2a77d3, 0x8250175ed792710f, 0x637ef20bd065422c, 0xa90eb02aa69ce297, 0x397bbdd6d513af17, 0xd35d180702c625df),
                  ("0x1.6acfde0000000p-8", "0x1.1ed3700000000p-13", "-0x1.1ed8ea0000000p-13", "0x1.0000000000000p+0", "0x0.0p+0")),
        "csr": ((0xf4312642d5ece3e5, 0x096940074e4097df, 0xe0e168d577dc6ac3, 0x874e3adf9778ec1f, 0x637ef20bd065422c, 0x9cb6f5b72f4af43f, 0xa90eb02aa69ce297, 0x397bbdd6d513af17, 0xd35d180702c625df),
                  ("0x0.0p+0", "0x1.1ed3700000000p-13", "-0x1.1ed8ea0000000p-13", "0x1.0000000000000p+0", "0x0.0p+0")),
    },
    "K16_d02": {
        "dense": ((0x0ca6fd8903e62d88, 0x3ada1a43eaa79e63, 0x49e5426fc6b94920, 0x7a385884c8b9d735, 0xcd95bb289824db0b, 0x4d25767f9dce13f5, 0xad2aca7747985764, 0xe15b0ce914a46769, 0xa9e50ab3db7c2174, 0x90ad52a43786ec9b),
                  ("0x1.d898c40000000p-10", "0x1.209d180000000p-14", "-0x1.24c62e0000000p-14", "0x1.d800000000000p-3", "0x0.0p+0")),
        "csr": ((0xdcc95184e097533b, 0x7aa6262db4a3da69, 0x10aa5aade3410634, 0xa8c7f832281a39c5, 0xad2aca7747985764, 0xe335e89b6f5b608d, 0xe15b0ce914a46769, 0xa9e50ab3db7c2174, 0x90ad52a43786ec9b),
                  ("0x0.0p+0", "0x1.209d180000000p-14", "-0x1.24c62e0000000p-14", "0x1.d800000000000p-3", "0x0.0p+0")),
    },
    "K16_d10": {
        "dense": ((0x3166612a67ab9bdf, 0x8b0315bfda7c707a, 0xf709ce98f53e00a4, 0xcc4ee6937f206ac4, 0xafa41d8ca364580c, 0x4d25767f9dce13f5, 0xad2aca7747985764, 0x6184e57dba15cb5a, 0xfdd928ce496f0b93, 0x8180dd6813dc2a62),
                  ("0x1.77d93c0000000p-9", "0x1.90b4be0000000p-14", "-0x1.90f0ea0000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
        "csr": ((0x4316e337fc9cc325, 0x79209b58ce80d790, 0x9e1b70b7c1dd6bdf, 0xa8c7f832281a39c5, 0xad2aca7747985764, 0xc852cd3db51120e7, 0x6184e57dba15cb5a, 0xfdd928ce496f0b93, 0x8180dd6813dc2a62),
                  ("0x0.0p+0", "0x1.90b4be0000000p-14", "-0x1.90f0ea0000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
    },
    "K17_d02": {
        "dense": ((0xa12bda262c854aa3, 0x8a929d5490363db2, 0x7bf2a2a4e66d000a, 0xd2ea2a2f0222ab62, 0x4e6e724c05d24631, 0xaa1cf61c9aab1585, 0x29c7dd317360ac35, 0x8ca09bd49bd81bf5, 0x600d2899fbd06e79, 0xcacd90804e32b487),
                  ("0x1.f67c280000000p-10", "0x1.ec4fb20000000p-15", "-0x1.ef16d40000000p-15", "0x1.6969696969697p-3", "0x0.0p+0")),
        "csr": ((0x7599370c5443e50a, 0x6ab57105375d7cfa, 0x4207e1f01b3a54cb, 0xc96e5d76a52cdc25, 0x29c7dd317360ac35, 0x38424b52afbae72a, 0x8ca09bd49bd81bf5, 0x600d2899fbd06e79, 0xcacd90804e32b487),
                  ("0x0.0p+0", "0x1.ec4fb20000000p-15", "-0x1.ef16d40000000p-15", "0x1.6969696969697p-3", "0x0.0p+0")),
    },
    "K17_d10": {
        "dense": ((0x911b325bf7ffec9c, 0xe92bf354b20c1e74, 0x7536f44cbe6035b5, 0x65b2c881d9b4d7f2, 0x12949156edf381de, 0xab71f4070d3bf145, 0xa6c82e33918d54e5, 0x26b8561346ea99a3, 0x568f59bb286760cb, 0xcd052639a44f2cfe),
                  ("0x1.d974ce0000000p-9", "0x1.686b160000000p-14", "-0x1.68b3cc0000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
        "csr": ((0x5fb8613470d57835, 0x5a384e494db53672, 0x911b325bf7ffec9c, 0x0abc9b33e95a53e5, 0xa6c82e33918d54e5, 0x9f23d4bd004dc821, 0x26b8561346ea99a3, 0x568f59bb286760cb, 0xcd052639a44f2cfe),
                  ("0x0.0p+0", "0x1.686b160000000p-14", "-0x1.68b3cc0000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
    },
    "K17_zero": {
        "dense": ((0xca05998bab3e6325, 0xc38543b30e36c325, 0xa05db089abcc6325, 0xf024277fb3c50b25, 0xcbf29ce484222325, 0xa8c7f832281a39c5, 0xa8c7f832281a39c5, 0xb5d23cc388d783ca, 0x62a10d0c038d7de6, 0x33dffa9ff736b263),
                  ("0x1.0000000000000p-149", "0x1.0000000000000p-149", "-0x1.0000000000000p+0", "0x0.0p+0", "0x0.0p+0")),
        "csr": ((0xcbf29ce484222325, 0xcbf29ce484222325, 0xcbf29ce484222325, 0x88201fb960ff6465, 0xa8c7f832281a39c5, 0xcbf29ce484222325, 0xb5d23cc388d783ca, 0x62a10d0c038d7de6, 0x33dffa9ff736b263),
                  ("0x0.0p+0", "0x1.0000000000000p-149", "-0x1.0000000000000p+0", "0x0.0p+0", "0x0.0p+0")),
    },
    "K300_d02": {
        "dense": ((0x03e4f39f1b646bc4, 0xbc3a956ceea2c609, 0xcd9b7ad8fb34f9b2, 0xee850a268a2b8cc4, 0xcb27d2b169d112b7, 0xcda8103eccbab189, 0x7dec3448a6345233, 0x1b5fed78c193dcc3, 0x9d16c377d3280006, 0x12fff584c09687f1),
                  ("0x1.cc34600000000p-8", "0x1.28020c0000000p-13", "-0x1.2804c80000000p-13", "0x1.9c31b2b8ddbafp-3", "0x0.0p+0")),
        "csr": ((0xb2f6b77572c9ae0a, 0x915a520e786c0cc0, 0x7b8e0b7e3669c41c, 0xa0cf076d9ceba699, 0x7dec3448a6345233, 0x76393537191970ac, 0x1b5fed78c193dcc3, 0x9d16c377d3280006, 0x12fff584c09687f1),
                  ("0x0.0p+0", "0x1.28020c0000000p-13", "-0x1.2804c80000000p-13", "0x1.9c31b2b8ddbafp-3", "0x0.0p+0")),
    },
    "K300_d10": {
        "dense": ((0xb31c87f73f892783, 0x3df658abfe9e08bd, 0xaeb2c544381c0c6d, 0xee5716a5dbc029a5, 0x8002429cf52c89fd, 0xf4892221028bb75e, 0x06b9a65968658126, 0x279628081737dc05, 0x574959eb5b370a27, 0xc5be117a3744ac60),
                  ("0x1.e9de800000000p-8", "0x1.67c0600000000p-13", "-0x1.67c07e0000000p-13", "0x1.0000000000000p+0", "0x0.0p+0")),
        "csr": ((0x029113eb8b074675, 0x7009030fd53a06c1, 0x6b2b70c46417b783, 0xb7c51c60b1ed365e, 0x06b9a65968658126, 0xa18d99fcfebc30af, 0x279628081737dc05, 0x574959eb5b370a27, 0xc5be117a3744ac60),
                  ("0x0.0p+0", "0x1.67c0600000000p-13", "-0x1.67c07e0000000p-13", "0x1.0000000000000p+0", "0x0.0p+0")),
    },
    "K37_big": {
        "dense": ((0x21f0c82934a80fa1, 0x4a5e1adb06a6992b, 0x8dd4bcf388f09863, 0xdeaeafbd4e7bcf80, 0xf2da8adde4d0b4e2, 0xce5ab154a083556a, 0x40ee82196939bad7, 0x34b14bcf6c5e9eba, 0x40411400e2892008, 0xe817b16e3f49e48c),
                  ("0x1.ffe5140000000p-10", "0x1.bb82600000000p+2", "-0x1.50b43c0000000p-15", "0x1.fa63db5932ad3p-2", "0x1.0000000000000p+0")),
        "csr": ((0x578af4ff3d867187, 0x629944f3dd1ed88c, 0x9e3bddaafd7c001d, 0x3d74e04323dc2faa, 0x40ee82196939bad7, 0x387af519d2eef598, 0x34b14bcf6c5e9eba, 0x40411400e2892008, 0xe817b16e3f49e48c),
                  ("0x0.0p+0", "0x1.bb82600000000p+2", "-0x1.50b43c0000000p-15", "0x1.fa63db5932ad3p-2", "0x1.0000000000000p+0")),
    },
    "K37_d02": {
        "dense": ((0x325a75ba741ebd4e, 0xa1823b651e373a14, 0x2ba3d1b22aa59eeb, 0xaced2ea7869c8de5, 0x99051eae26c4cc0c, 0x985fea6c465f93d5, 0xde24483a76fbb974, 0x00d640e00120a57c, 0xa3551253bb27b40f, 0x7827bf02579f23d3),
                  ("0x1.f705e20000000p-10", "0x1.dfe01c0000000p-14", "-0x1.e0fd380000000p-14", "0x1.4c1bacf914c1cp-3", "0x0.0p+0")),
        "csr": ((0x80f3b1fc631d6b28, 0x6f2d440d45bd8525, 0x014772fd8497ca06, 0x3fb05257b29b2345, 0xde24483a76fbb974, 0x46e782e01802e06a, 0x00d640e00120a57c, 0xa3551253bb27b40f, 0x7827bf02579f23d3),
                  ("0x0.0p+0", "0x1.dfe01c0000000p-14", "-0x1.e0fd380000000p-14", "0x1.4c1bacf914c1cp-3", "0x0.0p+0")),
        "csr_zeros": ((0x80f3b1fc631d6b28, 0x6f2d440d45bd8525, 0x014772fd8497ca06, 0x3fb05257b29b2345, 0xde24483a76fbb974, 0xfa5643a53f4a6d5e, 0x00d640e00120a57c, 0xa3551253bb27b40f, 0x7827bf02579f23d3),
                  ("0x0.0p+0", "0x1.dfe01c0000000p-14", "-0x1.e0fd380000000p-14", "0x1.4c1bacf914c1cp-3", "0x0.0p+0")),
    },
    "K37_d10": {
        "dense": ((0x21849d7edd2bdf9c, 0x805afb9dd255298a, 0x61338e52b4a8d312, 0x65ed0a3f2d3438e5, 0xe3959c844b631ead, 0x0cfef33cff8f15aa, 0xcaab1979c3250fb6, 0x6641da8dea24d639, 0x625251c143cd3198, 0x3aa9dbfb013ae6d9),
                  ("0x1.b14e260000000p-8", "0x1.3ba11c0000000p-13", "-0x1.3bdd8c0000000p-13", "0x1.b056c45902ce1p-1", "0x0.0p+0")),
        "csr": ((0xbfef08a958d416a5, 0x7f8b565a2c645505, 0x83c33c72e5f732b8, 0x008be9b8e6f10eea, 0xcaab1979c3250fb6, 0x9d0717ca7c181eb4, 0x6641da8dea24d639, 0x625251c143cd3198, 0x3aa9dbfb013ae6d9),
                  ("0x0.0p+0", "0x1.3ba11c0000000p-13", "-0x1.3bdd8c0000000p-13", "0x1.b056c45902ce1p-1", "0x0.0p+0")),
        "csr_zeros": ((0xbfef08a958d416a5, 0x7f8b565a2c645505, 0x83c33c72e5f732b8, 0x008be9b8e6f10eea, 0xcaab1979c3250fb6, 0x8780575aabbe39e4, 0x6641da8dea24d639, 0x625251c143cd3198, 0x3aa9dbfb013ae6d9),
                  ("0x0.0p+0", "0x1.3ba11c0000000p-13", "-0x1.3bdd8c0000000p-13", "0x1.b056c45902ce1p-1", "0x0.0p+0")),
    },
    "K5_d02": {
        "dense": ((0x2f04d903e3e5d32f, 0xcc3b71f161240ae0, 0xd2caff5b0162b634, 0xf07bb606e847a243, 0x340c814b8daa0102, 0x4d25767f9dce13f5, 0xad2aca7747985764, 0x79d8b96cb8719d0a, 0xf0f00ad26d7d5d24, 0xee902f12204f034b),
                  ("0x1.8aad380000000p-11", "0x1.8d92e40000000p-16", "-0x1.b3fec60000000p-16", "0x1.eb851eb851eb8p-3", "0x0.0p+0")),
        "csr": ((0x324593d307837bb4, 0xe8ea95fc3bc522ff, 0xf039dc9183a7eb23, 0xa8c7f832281a39c5, 0xad2aca7747985764, 0x3826896bbf40601b, 0x79d8b96cb8719d0a, 0xf0f00ad26d7d5d24, 0xee902f12204f034b),
                  ("0x0.0p+0", "0x1.8d92e40000000p-16", "-0x1.b3fec60000000p-16", "0x1.eb851eb851eb8p-3", "0x0.0p+0")),
    },
    "K5_d10": {
        "dense": ((0xe867278696856e6b, 0xdb58dd36cdcafe88, 0x1af25b2434625550, 0x2deb95371ca937c4, 0x0ac80e3048001890, 0x4d25767f9dce13f5, 0xad2aca7747985764, 0xad6cde415ba4d71d, 0x46eecff56eb5c747, 0x0121dfb4ee85ae6a),
                  ("0x1.b2fd440000000p-10", "0x1.1179680000000p-14", "-0x1.167f180000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
        "csr": ((0x725fed1430846021, 0x6aef611359aad73c, 0x51869bf22ee9ce6b, 0xa8c7f832281a39c5, 0xad2aca7747985764, 0x5861e7729c2734aa, 0xad6cde415ba4d71d, 0x46eecff56eb5c747, 0x0121dfb4ee85ae6a),
                  ("0x0.0p+0", "0x1.1179680000000p-14", "-0x1.167f180000000p-14", "0x1.0000000000000p+0", "0x0.0p+0")),
    },
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_tables_and_parameters_equal_the_recorded_ones(name):
    got = forms(name)
    assert sorted(got) == sorted(EXPECTED[name])
    for form, (rc, detail, digests, params) in got.items():
        assert (rc, detail) == (0, ""), (form, detail)
        names = decoder.MODEL_DIGESTS_DENSE if form == "dense" else decoder.MODEL_DIGESTS_CSR
        want_digests, want_params = EXPECTED[name][form]
        assert [digests[n] for n in names] == list(want_digests), form
        assert [float(params[p]).hex() for p in decoder.MODEL_PARAMS] == list(want_params), form


@pytest.mark.parametrize("name", sorted(MODELS))
def test_dense_and_csr_builders_agree(name):
    got = forms(name)
    _, _, dd, dp = got.pop("dense")
    for form, (_, _, cd, cp) in got.items():
        assert [cd[n] for n in SHARED_DIGESTS] == [dd[n] for n in SHARED_DIGESTS], form
        assert [cp[p] for p in SHARED_PARAMS] == [dp[p] for p in SHARED_PARAMS], form


def test_the_shapes_cover_what_they_claim():
    _, _, _, p = forms("K37_big")["dense"]
    assert p["any_big"] == 1.0 and MODELS["K37_big"][0].max() > 1 and MODELS["K37_big"][0].max() <= 50
    _, _, _, p = forms("K17_zero")["dense"]
    assert (p["qscale"], p["windowq"], p["density"]) == (-1.0, float(np.nextafter(np.float32(0), np.float32(1))), 0.0)
    A = MODELS["K37_d02"][0]
    for k in (0, 18, 36):
        assert not A[k].any() and not A[:, k].any()
    indptr, _, data = csr_with_stored_zeros(A, seed=37)
    assert (data == 0).sum() > 0 and indptr[-1] == data.size


# ---- refusals: the return code and the sentence

BAD_TEXT = "model entries must be finite and >= 0"
K0, M0 = 8, 3


def base():
    A, B, Pi = make_model(K0, M0, 1.0, seed=99)
    return A, B, Pi


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf")], ids=["negative", "nan", "inf"])
@pytest.mark.parametrize("which", ["A", "B", "Pi"])
def test_a_bad_entry_is_refused_by_both_builders(which, bad):
    A, B, Pi = base()
    {"A": A, "B": B, "Pi": Pi}[which].reshape(-1)[K0 * 4 + 1 if which == "A" else 5] = bad         # (A: row 4)
    rc, detail, _, _ = decoder.test_model_digest(A, B, Pi)
    assert (rc, detail) == (ERR_ARG, BAD_TEXT)
    rc, detail, _, _ = decoder.test_model_digest(decoder.dense_to_csr(A), B, Pi)
    # the stored entries are checked row by row, and the sentence names the row
    assert (rc, detail) == (ERR_ARG, BAD_TEXT + (" (row 4)" if which == "A" else ""))


def csr_case(edit):
    A, B, Pi = base()
    indptr, indices, data = decoder.dense_to_csr(A)
    edit(indptr, indices, data)
    return decoder.test_model_digest((indptr, indices, data), B, Pi)[:2]


def test_csr_array_refusals():
    who = "fv_set_model_sparse: "

    def first(ip, ix, d):
        ip[0] = 1
    assert csr_case(first) == (ERR_ARG, who + "row_ptr[0] must be 0 (row 0)")

    def decreasing(ip, ix, d):
        ip[4] = ip[3] - 1
    assert csr_case(decreasing) == (ERR_ARG, who + "row_ptr decreases at row 3")

    def col_k(ip, ix, d):
        ix[ip[6] + K0 - 1] = K0
    assert csr_case(col_k) == (ERR_ARG, who + "row 6 holds a column outside [0, K)")

    def col_negative(ip, ix, d):
        ix[ip[1]] = -1
    assert csr_case(col_negative) == (ERR_ARG, who + "row 1 holds a column outside [0, K)")

    def equal_columns(ip, ix, d):
        ix[ip[2] + 3] = ix[ip[2] + 2]
    assert csr_case(equal_columns) == (ERR_ARG, who + "the columns of row 2 are not strictly ascending")

    def bad_value(ip, ix, d):
        d[ip[4] + 2] = -1.0
    assert csr_case(bad_value) == (ERR_ARG, BAD_TEXT + " (row 4)")

    # two faults: the rows are reported in ascending order, whatever the fault — row 2's order before row 5's range
    def two(ip, ix, d):
        ix[ip[5] + 1] = K0 + 3
        ix[ip[2] + 3] = ix[ip[2] + 2]
    assert csr_case(two) == (ERR_ARG, who + "the columns of row 2 are not strictly ascending")

    # ... and inside one row the range before the order
    def two_in_a_row(ip, ix, d):
        ix[ip[5] + 1] = K0 + 3
        ix[ip[5] + 4] = ix[ip[5] + 3]
    assert csr_case(two_in_a_row) == (ERR_ARG, who + "row 5 holds a column outside [0, K)")

    # a bad column is reported before a bad value, whatever their rows
    def column_and_value(ip, ix, d):
        d[ip[1]] = float("nan")
        ix[ip[6]] = -1
    assert csr_case(column_and_value) == (ERR_ARG, who + "row 6 holds a column outside [0, K)")
