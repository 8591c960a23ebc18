"""Mapped mode (include/tyr_c.h "Adaptive sampling") modelled on the oracle alone, so that a HIP ctx in mapped mode has a
specification to be compared with that is not another HIP ctx.

The oracle has no sample maps and needs none.  A fresh camera-ray record is a constant apart from origin, direction and pixel
(direct = 1, distance = 0, identifier = 0, bounces = 0, geometry_type = 1, lastSpecular = 1); adaptive_ref.camera_rays restates
those three (pinned bit for bit to the oracle's first wavefront by test_adaptive) and adaptive_ref.ticket_pixels the ticket list.
One mapped iteration is then the oracle's own iteration with its primary stage replaced:

    surv = the survivors `begin` left;  nNew = min(N - surv, b)           (b: the model's budget_remaining)
    the oracle's primary stage with a budget of exactly nNew              (it lays down nNew raster rays behind the survivors and
                                                                            does set_wavefront_globals: n_live, start_position
                                                                            advanced by nNew, total_primary_rays, total_extend_rays)
    the nNew raster records replaced by the restated rays of tickets T - b .. T - b + nNew - 1 at launch indices 0 .. nNew - 1
    b -= nNew;  extend, shade, connect, end as they are.

Letting the oracle count its own raster rays before they are replaced is what the header asks for: "start_position still
advances by the rays made, mod P; mapped mode does not read it".  (A model that keeps the oracle's budget at 0 and imports the
queue in front of the primary stage computes the same images but leaves start_position behind, and the first tyr_render after
the mode ends would start at another pixel than the HIP ctx does.)  The records are replaced with import_work_queue(queue, n)
followed by import_work_queue(queue, 0): the first copies them in, the second puts primary_ray_cnt back to the 0 the primary
stage left, which shade counts the survivors from.

MappedOracle has the Oracle's interface, so a caller that drives an Oracle can drive it unchanged; test_mapped_model.py pins it
on the CPU, which is the guard that the model, not the GPU, is the specification."""
from __future__ import annotations

import numpy as np

import adaptive_ref as ar

STAGES = ("begin", "primary", "extend", "shade", "connect", "end")


class MappedOracle:
    def __init__(self, oracle, camera, rank=0, nranks=1):
        from oracle import pyorc

        self.o = oracle
        self.lib = pyorc.lib()
        self.W, self.H, self.N = oracle.W, oracle.H, oracle.N
        self.rank, self.nranks = rank, nranks
        self.cam = camera  # (what load_scene set: the model makes the camera rays itself)
        self.mapped = False
        self.local = np.zeros(0, np.int64)  # the map on the ctx's rows
        self.T = 0
        self.b = 0  # budget_remaining while the mode lasts

    def __getattr__(self, name):  # everything that mapped mode does not touch: upload, reset_accum, the queues, ...
        return getattr(self.o, name)

    # ---- the mode ----
    def set_sample_map(self, m) -> int:
        m = np.asarray(m)
        assert m.shape == (self.H, self.W) and m.min(initial=0) >= 0 and m.max(initial=0) <= 65535
        self.local = ar.local_rows(m, self.rank, self.nranks).astype(np.int64)
        self.T = self.b = int(self.local.sum())
        self.mapped = True
        return self.T

    def set_budget(self, n):
        self.mapped = False  # "Mapped mode lasts until tyr_set_budget or tyr_render set a budget of their own"
        self.o.set_budget(n)

    def render(self, spp, max_iterations=1 << 30):
        self.mapped = False
        return self.o.render(spp, max_iterations)

    def set_camera(self, cam):
        self.cam = cam
        self.o.set_camera(cam)

    def counters(self) -> dict:
        k = self.o.counters()
        if self.mapped:
            k["budget_remaining"] = self.b
        return k

    # ---- an iteration ----
    def new_rays(self, first_ticket, n, frame):
        """the records of tickets first_ticket .. first_ticket + n - 1 at launch indices 0 .. n - 1"""
        from tyrant_amd.scenes import RAY_DTYPE

        pix = ar.ticket_pixels(self.local, first_ticket, n)
        assert pix.size == n, (pix.size, n)
        origin, direction, index = ar.camera_rays(self.lib, self.cam, self.W, self.H, pix, np.arange(n), frame, self.rank, self.nranks)
        q = np.zeros(n, RAY_DTYPE)
        q["origin"], q["direction"], q["index"] = origin, direction, index
        q["direct"], q["geometry_type"], q["lastSpecular"] = 1.0, 1, 1
        return q

    def stage(self, name):
        if not self.mapped or name != "primary":
            return self.o.stage(name)
        k = self.o.counters()
        surv = k["primary_ray_cnt"]
        n_new = min(self.N - surv, self.b)
        self.o.set_budget(n_new)
        if n_new:
            q = np.concatenate([self.o.ray_queue(0, surv), self.new_rays(self.T - self.b, n_new, k["frame"])])
        self.o.stage("primary")
        if n_new:
            self.o.import_work_queue(q, surv + n_new)
            self.o.import_work_queue(q, 0)
        self.b -= n_new

    def launch_kernels(self):
        if not self.mapped:
            return self.o.launch_kernels()
        for st in STAGES:
            self.stage(st)
        return 0

    def render_adaptive(self, m, max_iterations=1 << 30) -> int:
        """tyr_set_sample_map, then orc_render's loop on that budget"""
        self.set_sample_map(m)
        it = 0
        while it < max_iterations:
            self.launch_kernels()
            it += 1
            if self.b == 0 and self.o.counters()["primary_ray_cnt"] == 0:
                break
        return it


def maps(H, W, rng):
    """the kinds of map the sequences use"""
    P = H * W
    sparse = np.zeros((H, W), np.int32)
    k = max(P // 40, 3)
    sparse.reshape(-1)[rng.choice(P, size=k, replace=False)] = rng.integers(1, 7, size=k)
    one = np.zeros((H, W), np.int32)
    one.reshape(-1)[int(rng.integers(0, P))] = 3000
    one.reshape(-1)[:: max(P // 7, 1)] += 1
    return {
        "uniform1": np.full((H, W), 1, np.int32),
        "uniform2": np.full((H, W), 2, np.int32),
        "random": rng.integers(0, 5, size=(H, W)).astype(np.int32),
        "sparse": sparse,
        "one_large": one,
        "zero": np.zeros((H, W), np.int32),
    }
