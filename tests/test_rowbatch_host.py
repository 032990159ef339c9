"""The shape of the batched front ends: one iteration core, rowbatch.RowBatch, under FitBatch, CtVolume, InpaintBatch
and SiblingBatch; what the core owns is defined once, and a one-launch batch is the one-group case of the group loop."""
import pytest


def test_the_four_batches_share_one_core():
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd.rowbatch import ElboRowBatch, RowBatch
    four = (M.FitBatch, M.CtVolume, M.InpaintBatch, M.SiblingBatch)
    assert all(issubclass(c, RowBatch) for c in four)
    assert all(issubclass(c, ElboRowBatch) for c in (M.FitBatch, M.CtVolume, M.InpaintBatch))
    assert issubclass(ElboRowBatch, RowBatch) and not issubclass(M.SiblingBatch, ElboRowBatch)
    for c in four:
        for name in ("fit", "_wait_ema", "_ema", "grad_only", "step", "dead", "predict", "metrics", "init_params", "to_engine"):
            assert name not in vars(c), (c.__name__, name)
            assert name in vars(RowBatch), name
    assert M.CtVolume.task == "ct" and M.InpaintBatch.task == "inp"      # (FitBatch and SiblingBatch: the constructor's den / sr)


def test_helpers_live_in_rowbatch_and_keep_their_old_names():
    from mfvi_dip_mia_amd import ctvolume, fitbatch, rowbatch
    for name in ("per_fit", "prior_sigmas", "EXP_WEIGHT", "TASKS"):
        assert getattr(fitbatch, name) is getattr(rowbatch, name), name
    assert ctvolume.groups is rowbatch.groups and ctvolume.MAX_LAUNCH == rowbatch.MAX_LAUNCH == 65535


@pytest.mark.parametrize("F,K", [(1, 1), (2, 1), (3, 2), (16, 1), (4, 16)])
def test_a_one_launch_batch_is_one_group(F, K):
    from mfvi_dip_mia_amd.rowbatch import groups
    assert groups(F, F, K) == [(0, F, 0, 0, F * K)]
