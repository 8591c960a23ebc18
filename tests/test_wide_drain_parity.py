"""The drain four lanes to a ray (k_trace_flat -> wide_drain) against the oracle, with the wide drain on and off.  Needs an
MI355X: `pytest -m gpu`.

Small queues on trees deeper than the LDS stack: every wave holds a few dozen rays at most, the queue is used up after its
first draws, and the long rays of every wave -- most of a launch's node steps -- are finished four lanes to a ray.  Queues
must stay bit-identical to the oracle's (DESIGN.md "Numeric contract"), whichever way a wave's last rays are traced."""
import numpy as np
import pytest

from conftest import bits, built_scene

pytestmark = pytest.mark.gpu


def _pair(orc, hip, name, W, H, N):
    sc, nodes, prims = built_scene(name)
    flags = (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)
    o = orc.Oracle(W, H, N, flags=flags & 25)
    o.load_scene(sc, nodes, prims)
    g = hip.Renderer(W, H, N, flags=flags)
    g.load_scene(sc, nodes, prims)
    return o, g


@pytest.mark.parametrize("name,W,H,N", [("mesh128", 48, 32, 1500), ("cornell_soup2k", 40, 24, 960), ("glass_dof48", 48, 27, 1296)])
@pytest.mark.parametrize("wide_drain", [1, 0])
def test_small_queues_match_the_oracle_with_and_without_the_wide_drain(orc, hip, name, W, H, N, wide_drain):
    o, g = _pair(orc, hip, name, W, H, N)
    assert g.scene_info()["quad_max_stack"] <= 48, name  # (a deeper tree keeps its rays one to a lane: the two runs would be the same)
    g.set_tuning(wide_drain=wide_drain, wide_block_min_items=0)  # (also the 768-thread form of the kernel: six waves per SIMD)
    for it in range(4):
        o.launch_kernels(), g.launch_kernels()
        ko, kg = o.counters(), g.counters()
        assert kg["device_error"] == 0, kg
        for f in ("primary_ray_cnt", "shadow_ray_cnt", "n_shadow_visible", "total_shadow_rays", "n_survive"):
            assert ko[f] == kg[f], (name, wide_drain, it, f, ko[f], kg[f])
        ns, nh = ko["primary_ray_cnt"], ko["shadow_ray_cnt"]
        qo, qg = o.ray_queue(0, ns), g.ray_queue(0, ns)
        for f in ("origin", "direction", "direct"):
            assert np.array_equal(bits(qo[f]), bits(qg[f])), (name, wide_drain, it, f)
        for f in ("index", "bounces", "lastSpecular"):
            assert np.array_equal(qo[f], qg[f]), (name, wide_drain, it, f)
        assert o.shadow_queue(nh).tobytes() == g.shadow_queue(nh).tobytes(), (name, wide_drain, it)
    bo, bg = o.blit_buffer(), g.blit_buffer()
    assert np.array_equal(bo[:, 3], bg[:, 3])
    assert np.allclose(bg[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,W,H,N,spp", [("mesh128", 64, 36, 2304, 3), ("cornell_area_light", 48, 32, 1536, 3)])
def test_renders_match_the_oracle_with_and_without_the_wide_drain(orc, hip, name, W, H, N, spp):
    o, g1 = _pair(orc, hip, name, W, H, N)
    _, g0 = _pair(orc, hip, name, W, H, N)
    assert g1.scene_info()["quad_max_stack"] <= 48, name
    g1.set_tuning(wide_drain=1)
    g0.set_tuning(wide_drain=0)
    io, i1, i0 = o.render(spp), g1.render(spp), g0.render(spp)
    assert io == i1 == i0
    ko, k1, k0 = o.counters(), g1.counters(), g0.counters()
    assert k1["device_error"] == 0 and k0["device_error"] == 0
    for f in ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible"):
        assert ko[f] == k1[f] == k0[f], (name, f)
    bo = o.blit_buffer()
    for bg in (g1.blit_buffer(), g0.blit_buffer()):
        assert np.array_equal(bo[:, 3], bg[:, 3])
        assert np.allclose(bg[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6)
