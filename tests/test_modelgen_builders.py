"""CPU: the model builders of tests/modelgen.py return, bit for bit, what they returned before every kind got its one
construction behind model64 / model32.  The hashes (modelgen.sha of A, B, Pi, and of ob where the builder draws it) were
recorded at the commit before that change, for every instance the suite builds (T of the step-table instances: the
length their pass sets need, 50 at K = 600 and 52 at K = 300) and for the two rotors of the golden fixtures.

Also: a spec of each new kind gives the builder's arrays through model32, and the float32 circulant model survives the
'%.16f' text of its widening unchanged, so the fixture's reference binaries read exactly the arrays the GPU tests use."""
import numpy as np
import pytest

import modelgen
from flash_viterbi_amd import hostio

RECORDED = [
    ('wide_model', ('wideA', 600, 6, 60, 401), ('73eedf43de5425c5', '99dc8e0ad60e5f17', 'b743c791c52b820e', 'ed6ee53321a0b87c')),
    ('wide_model', ('wideB', 600, 6, 60, 402), ('232db704db1cfc99', 'd72411c0be98cc72', 'b716e504b5ec0a0b', 'bcb5692348c2ad53')),
    ('wide_model', ('wideAB', 600, 6, 60, 403), ('4102dbdef779af70', '74e38a7963cfa73c', '12369c3306d1df37', '0f36f606bbe858c4')),
    ('wide_model', ('wideA', 4500, 5, 24, 404), ('625c68c977075730', 'b911b4d25a7ba821', '4be3d8cdc3341b97', '1af3026f36d937a7')),
    ('wide_model', ('wideB', 4500, 5, 24, 405), ('58f537da7a9e29a5', '5eca81c667998f0f', 'a4cd1dc5e7f525d3', 'cc1825de02651373')),
    ('wide_model', ('wideA', 600, 6, 60, 411), ('6e93d1f449347e0c', '90f10a101931b444', '3155ca6b50fe5e39', '2594827094baecbb')),
    ('wide_model', ('wideB', 600, 6, 60, 412), ('441af32c422fa1a7', 'c145a22f22e8e234', 'c237e1cc29714be8', '6ad706e90b390af8')),
    ('wide_model', ('wideAB', 600, 6, 60, 413), ('0ad7fc50b9c8a10b', '62d67544383ed0aa', '0b627364f4ad3fef', 'b262b7334eea519a')),
    ('wide_model', ('wideB', 4500, 5, 24, 414), ('06bc0a3c3fe9aace', 'e1d957d6f5d5d7ba', '52334b18b0d5e356', '620c8ecb8d56d418')),
    ('wide_model', ('wideB', 600, 8, 50, 1000), ('1c663cdd96e60b6c', '8ec9b9a72db85977', 'da67cf70fb98e5e1', '0578edae40c933d3')),
    ('wide_model', ('wideA', 600, 8, 50, 1000), ('fcd4ce0a2b8ec2d1', '52ba29384e946631', '6c2aef7fa1050a10', '166e9d0594d79914')),
    ('wide_model', ('wideB', 600, 8, 48, 5), ('728b9a59b91936d2', 'beedfd507af5ef23', '8d957950fd319774', '56b8392f4f13168b')),
    ('wide_model', ('wideAB', 600, 8, 48, 5), ('f6b7dc5e591fe97b', 'fc2d9859c97d8ab9', 'f2fa69040fc3aad5', 'dbc0cd573a35030b')),
    ('wide_model', ('wideB', 257, 8, 90, 6), ('387fc803b2802ff0', '2f74751f8289bbc9', '35270ec401fb4dde', '5b95c87ab1c100bb')),
    ('wide_model', ('wideAB', 257, 8, 90, 6), ('ff3ec3f21069167b', 'd7286bb6a9077ca0', 'e3431b8feb3c3665', '1741c3d227496b04')),
    ('wide_model', ('wideA', 600, 6, 4, 1600), ('e0e88ae1d373eae1', '08b91ae9292c7c41', '48e88d6a70d2d175', 'aaf989d66d3b12a4')),
    ('wide_model', ('wideA', 600, 6, 4, 1130), ('2cb6807aa53c89d6', '62462166813b56f3', 'afb0411855e93eec', '90bb68ec5276c74e')),
    ('wide_model', ('wideA', 600, 6, 4, 1164), ('37cce2cc5cc8010b', '16062f0a4e0d6c45', '11970df26cb3a120', '6443e49718280c45')),
    ('wide_model', ('wideA', 600, 6, 4, 1200), ('84cf5830ad3b11ec', '06511c4d7005f106', '63013121bb56e250', 'fc5b95552c5740a8')),
    ('wide_model', ('wideA', 600, 6, 4, 1357), ('d1080797b2d981f3', '4be6ef1a978187ba', '90da66ec9b805f5a', 'c5cae7a08b2a0bc9')),
    ('wide_model', ('wideA', 300, 10, 200, 77), ('e85ea44841544ae3', 'dae7005b9f597c21', 'bfcf0f9ee936c952', '5b05d976d6cc77de')),
    ('wide_model', ('wideB', 300, 10, 200, 77), ('3e0f46d1860ea0c6', 'e721b102e5a1648d', 'cbc1c91432f69f11', '5ac66691295e05ce')),
    ('wide_model', ('wideAB', 300, 10, 200, 77), ('f6951fb17a6ae43a', '4fedca9c3e8bfbef', '678335ab80445469', 'e6e6d0fb7e61760a')),
    ('rotor', (61, 7, 0, 161), ('9e2812e501991f96', '7ba74fa38b70e824', '8d06bd6722e1ab1b')),
    ('rotor', (61, 7, 0.02, 161), ('a58acab3963822ea', 'b56339410b674ba6', 'fdb8fc511d936539')),
    ('rotor', (61, 7, 0.2, 161), ('e2954b87cedd7753', 'b56339410b674ba6', 'fdb8fc511d936539')),
    ('rotor', (257, 7, 0, 357), ('9b7034ae735a0ff5', 'cfca83acfb07f45b', 'be7b13516bff190f')),
    ('rotor', (257, 7, 0.02, 357), ('4210c60243b2b9e1', '44c5030f3f79d1ef', '03a3f572fb15035e')),
    ('rotor', (257, 7, 0.2, 357), ('855993b3788dbf9c', '44c5030f3f79d1ef', '03a3f572fb15035e')),
    ('rotor', (193, 7, 0, 293), ('62d5fe1c3eb36d5e', 'ed57e62334c66487', '619f2129d50af33e')),
    ('rotor', (193, 7, 0.01, 293), ('842a3a52ecf68ee3', 'ece75779c081022c', 'f192706b51e27299')),
    ('rotor_tied_column', (131, 30), ('fda48c968d2e6232', 'f85c35ff2552d392', '8c820a59a1f497fa')),
    ('rotor_tied_column', (), ('fda48c968d2e6232', 'f85c35ff2552d392', '8c820a59a1f497fa')),
    ('circulant_ties', (257,), ('e44acef813161a29', '988ae6e409f85dea', '811953bbedff46c6')),
    ('circulant_ties', (1025,), ('85a71ff8b6f70ad7', 'e17c4a91a9bea518', 'be1e49d21683e418')),
    ('circulant_ties', (2053,), ('832f898ec963b3c0', '7883112ddbe4e7b4', '774d6727c9497124')),
    # tests/test_gpu_step_tables.py's unreachable_model before it moved; tests/test_gpu_sparse_model.py's, likewise
    ('unreachable_model', (300, 8, 52, 700), ('5dd4d4abc9865ddf', 'a89b0d73f1128f95', '94ef7aa68b6f6f60', '537955fed95e46cd')),
    ('unreachable_fast', (300, 8, 52, 700), ('e717447a88cf2d0b', '6b8dda33c6340f35', '94ef7aa68b6f6f60', '537955fed95e46cd')),
]


@pytest.mark.parametrize("builder,args,want", RECORDED, ids=[f"{b}{a}".replace(" ", "") for b, a, _ in RECORDED])
def test_builder_returns_the_recorded_bits(builder, args, want):
    got = getattr(modelgen, builder)(*args)
    assert len(got) == len(want)
    assert all(x.dtype == np.float32 for x in got[:3]) and all(x.dtype == np.int32 for x in got[3:])
    assert tuple(modelgen.sha(x) for x in got) == want


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


def test_specs_give_the_builders_arrays():
    ob = [0, 1, 1, 0]
    spec = modelgen.wide_spec("wideB", 257, 8, 90, 6)
    assert same(modelgen.model32(spec), modelgen.wide_model("wideB", 257, 8, 90, 6))
    spec = dict(kind="rotor", K=61, M=7, T=4, prob=0.5, noise=0.02, seed=161, ob=ob)
    assert same(modelgen.model32(spec)[:3], modelgen.rotor(61, 7, 0.02, 161))
    spec = dict(kind="rotor_tied_column", K=131, M=2, T=4, prob=0.5, g=30, ob=ob)
    assert same(modelgen.model32(spec)[:3], modelgen.rotor_tied_column(131, 30))
    spec = dict(kind="unreachable", K=300, M=8, T=4, prob=0.112, seed=700, ob=ob)
    assert same(modelgen.model32(spec)[:3], modelgen.unreachable_model(300, 8, 4, 700)[:3])
    assert modelgen.model32(spec)[3].tolist() == ob


@pytest.mark.parametrize("K", sorted(modelgen.CIRCULANT_OFF))
def test_circulant_float32_survives_the_text_round_trip(K, tmp_path):
    """model64 is the widening of the float32 arrays; quantize_text16 of it, and the text files themselves parsed as the
    loader does (strtod, then a cast to float), give the float32 arrays back."""
    built = modelgen.circulant_ties(K)
    spec = dict(kind="circulant_ties", K=K, M=10, T=3, prob=0.5, ob=[0, 8, 9])
    wide = modelgen.model64(spec)
    assert all(w.dtype == np.float64 and np.array_equal(w, b) for w, b in zip(wide, built))
    assert same(modelgen.model32(spec)[:3], built)
    assert same([hostio.quantize_text16(w) for w in wide], built)
    if K == min(modelgen.CIRCULANT_OFF):
        modelgen.write_text(spec, str(tmp_path))
        for name, b in zip(("A", "B", "Pi"), built):
            text = np.loadtxt(tmp_path / f"{name}_K{K}_T3_prob0.5.txt", dtype=np.float64, ndmin=2)
            assert same([text.astype(np.float32).reshape(b.shape)], [b]), name
