"""pbrs_upload_scene refuses before it touches the device: a refused upload leaves the context's scene in place."""
import types

import pytest

import pbrs_amd
from pbrs_amd import api, scenes
from common import bits

pytestmark = pytest.mark.gpu


def test_a_refused_upload_leaves_the_previous_scene_in_place(gpu_ctx):
    hs = pbrs_amd.HostScene(scenes.build_config("c2", width=32, height=32)[0])
    gpu_ctx.upload(hs)
    first, _ = gpu_ctx.render(1, 1, 3, seed=7)
    bad = api.SceneDesc.from_buffer_copy(hs.desc)  # the same arrays, an environment kind nobody knows
    bad.env_kind = 99
    with pytest.raises(pbrs_amd.PbrsError, match="unknown environment kind"):
        gpu_ctx.upload(types.SimpleNamespace(desc=bad))
    again, _ = gpu_ctx.render(1, 1, 3, seed=7)
    assert first.any() and (bits(first) == bits(again)).all()
