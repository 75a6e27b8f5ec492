"""Every option of a frame sequence at once (Context.render_animation with spatial, clip, upscale, display and motion vectors): the one
combination that none of the hand-made-chain tests of the single options covers, against the host variants called in the chain's
order."""
import numpy as np
import pytest

import motion_model as mm
import pbrs_amd
import temporal_model as tm
from common import bits
from pbrs_amd import api
from test_gpu_denoise import same
from test_gpu_display import gpu as displayed
from test_gpu_upsample import _by_hand

pytestmark = pytest.mark.gpu

f32 = np.float32


def test_render_animation_with_every_option_is_the_hand_made_chain(gpu_ctx):
    """The 32 x 32 Cornell box whose short box turns, traced at 16 x 16: three frames, so that the ping-pong halves swap twice and the
    exposure word and the motion table, first read on frame 1, are read again on frame 2.  Every returned image bit for bit."""
    tparams = dict(id_test=True, min_temporal=2.0)
    clip = dict(radius=2)
    scenes_ = [pbrs_amd.HostScene(mm.turned_short_box(k, size=32)) for k in range(3)]
    frames = list(gpu_ctx.render_animation([(hs, None, 9 + k) for k, hs in enumerate(scenes_)], 2, 2, 5, temporal=tparams, spatial=True, clip=clip,
                                           upscale=2, display=True, motion_vectors="prev_depth", iterations=3))
    assert len(frames) == 3
    history = prev = cam_prev = e = None
    for k, (hs, (full, acc, noisy, st, mv)) in enumerate(zip(scenes_, frames)):
        gpu_ctx.upload(hs)
        table = api.instance_motion(hs, scenes_[k - 1]) if k else None
        cam_lo, img, aov, hi = _by_hand(gpu_ctx, hs.camera, 2, 5, 9 + k, 2)
        var = aov.pop("variance")
        kept = {n: aov[n] for n in tm.GUIDE_NAMES}
        history, v = gpu_ctx.temporal_accumulate(img, aov["depth"], cam_lo, variance=var, normal=aov["normal"], instance=aov["instance"], history=history,
                                                 prev=prev, camera_prev=cam_prev, motion=table, clip=clip, **tparams)
        v = gpu_ctx.spatial_variance(history["moments"], history["length"], v, min_temporal=2.0, **kept)
        den = gpu_ctx.denoise_var(history["rgb"], v, iterations=3, **aov)
        want = gpu_ctx.upsample(den, 32, 32, 2, lo=aov, hi=hi)
        e_prev = e
        shown, e, _ = displayed(gpu_ctx, want, exposure_in=e_prev, auto=True)
        assert full.shape == (32, 32, 3) and acc.shape == noisy.shape == (16, 16, 3) and st["low_res"] == (16, 16), k
        assert (bits(noisy) == bits(img)).all() and same(acc, history["rgb"]).all(), k
        assert same(full, want).all(), k
        assert st["display"].shape == (32, 32, 4) and st["display"].dtype == np.uint8 and (st["display"] == shown).all(), k
        assert f32(st["exposure"]).tobytes() == f32(e).tobytes(), k
        assert mv.shape == (16, 16, 3) and mv.dtype == f32, k
        if k:
            want_mv, want_wq = gpu_ctx.motion_vectors(aov["depth"], cam_lo, cam_prev, instance=aov["instance"], motion=table, return_prev_depth=True)
            assert same(mv[:, :, :2], want_mv).all() and same(mv[:, :, 2], want_wq).all(), k
        else:
            assert (bits(mv[:, :, :2]) == 0).all() and np.isposinf(mv[:, :, 2]).all()
        prev, cam_prev = kept, cam_lo
    box = aov["instance"] == mm.SHORT_BOX
    assert box.any() and np.abs(mv[:, :, :2][box]).max() > 0.0  # the table is read: the turning box moves on the film
