"""pt_render_with_di with frames in flight: the buffers a frame reads as its DI are held to the rotation rule of pt_render's buffers, so a
later frame on another lane that writes one of them (as its out) cannot overwrite it before the earlier frame's gather has read it."""
import numpy as np
import pytest

from test_denoiser_outputs import bits_equal
from test_restir_di import primary_hits, random_di, setup


@pytest.mark.gpu
def test_gpu_with_di_buffer_written_by_a_later_frame(dxrs, host):
    """write after read: a frame on another lane whose output is a buffer an earlier frame in flight reads as its DI must not overwrite
    it before that frame has read it"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 320, 180
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h), w, h, bounces=8, spp=1)
        hit = primary_hits(r, None)
        dev = torch.device("cuda", 0)
        d = random_di(np.random.default_rng(11), h, w)
        zero = torch.zeros((h, w, 4), device=dev)
        outs = [torch.full((h, w, 4), float("nan"), device=dev) for _ in range(3)]
        torch.cuda.synchronize(dev)
        r.render_with_di_device(outs[0].data_ptr(), zero.data_ptr(), zero.data_ptr())
        r.synchronize()
        res0 = outs[0].cpu().numpy()
        for k in range(4):
            dd = torch.from_numpy(d).to(dev)
            torch.cuda.synchronize(dev)
            r.render_with_di_device(outs[1].data_ptr(), dd.data_ptr(), zero.data_ptr())
            r.render_device(dd.data_ptr())  # the next lane's frame writes over the DI buffer
            r.render_device(outs[2].data_ptr())
            r.synchronize()
            want = res0.copy()
            want[..., :3] = np.where(hit[..., None], (res0[..., :3] + (d[..., :3] + np.float32(0))).astype(np.float32), res0[..., :3])
            bits_equal(outs[1].cpu().numpy(), want, f"round {k}: the DI as it was before the later frame wrote the buffer")
    finally:
        r.close()
