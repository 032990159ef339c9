"""The KL kernel family against the frozen output bits of tests/golden/kl_update_bits.npz: every entry point that
forms a KL term -- the fused updates (float32, guarded, bf16, per fit), the unfused gradients and sums, in the reverse and the forward
direction and against a mixture prior -- reproduces, bit for bit, what the separate kernels of before the fold wrote for the cases of
tests/klbits_cases.py (recorded by scripts/make_golden_klbits.py from a library built from the preceding commit's sources).

Bounds.  Digests (sha256 of an output array's raw bytes) and the one-block unfused sums: equality.  The unfused sums over several blocks end
in a float64 atomicAdd across blocks, whose last bits may depend on the order the blocks arrive in: klbits_cases.CLOSE_RTOL = 1e-10
relative, the bound of the unfused-vs-fused checks of tests/test_gpu_kl.py."""
import os

import numpy as np
import pytest

import klbits_cases as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "kl_update_bits.npz"), allow_pickle=False)
    digests = {k.decode(): bytes(v) for k, v in zip(z["digest_names"], z["digests"])}
    values = {k.decode(): float(v) for k, v in zip(z["value_names"], z["values"])}
    return digests, values


@pytest.fixture(scope="module")
def got(M):
    return K.record(M)


def test_the_record_covers_the_same_cases(got, gold):
    digests, exact, close = got
    assert sorted(digests) == sorted(gold[0])
    assert sorted(["exact/" + k for k in exact] + ["close/" + k for k in close]) == sorted(gold[1])


def test_every_output_array_has_the_frozen_bits(got, gold):
    wrong = sorted(k for k, d in got[0].items() if gold[0].get(k) != d)
    print("%d digests, %d differ" % (len(got[0]), len(wrong)))
    assert not wrong, wrong


def test_one_block_sums_have_the_frozen_bits(got, gold):
    for k, v in sorted(got[1].items()):
        ref = gold[1]["exact/" + k]
        print(k, repr(v), repr(ref))
        assert np.float64(v).tobytes() == np.float64(ref).tobytes(), k


def test_multi_block_sums_agree_to_the_atomic_order(got, gold):
    for k, v in sorted(got[2].items()):
        ref = gold[1]["close/" + k]
        err = abs(v - ref) / abs(ref)
        print(k, repr(v), repr(ref), err)
        assert err <= K.CLOSE_RTOL, (k, v, ref)
