"""CPU tests of the option knobs (mfh_set_option / mfh_get_option) on a host-only context: the literal list below is the contract -- every
name the library accepts, its default, what in-range values read back, what the setter clamps or maps, and what it rejects. The expected values
were written from the `else if` ladder that mfh_set_option was before the options moved into one table (and from the initialisers of mfh_ctx),
not from that table."""
import math
import os
import re

import pytest

import meshfem_amd as M
from meshfem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")

# name: (default, [(value set, value read back), ...], [rejected values])
OPTIONS = {
    "asm_chunk_order": (0, [(1, 1), (0, 0), (3.7, 3)], []),                       # plain int cast
    "mg_steps_fine": (1, [(3, 3), (0, 1), (-5, 1)], []),
    "mg_steps_coarse": (1, [(2, 2), (0, 1)], []),
    "mg_ratio_fine": (0.3, [(0.5, 0.5), (1e-3, 1e-3)], [0, 1, -0.1, 1.5]),
    "mg_ratio_coarse": (0.3, [(0.25, 0.25)], [0, 1]),
    "mg_coarse_cycles": (1, [(2, 2), (0, 1)], []),
    "placement_trials": (0, [(3, 3), (99, 8), (-1, 0)], []),
    "mg_eig_margin": (1.1, [(1.0, 1.0), (2.5, 2.5)], [0.5, 0.999]),
    "mg_agg_target": (32, [(16, 16), (-3, 0)], []),
    "mg_coarse_fp32": (1, [(0, 0), (5, 1)], []),
    "mg_over_correction": (1.5, [(2.0, 2.0)], [0, 4, -1]),
    "mg_dense_max": (1200, [(500, 500), (3, 8)], []),
    "mg_steps_agg": (2, [(4, 4), (0, 1)], []),
    "mg_ratio_agg": (0.2, [(0.4, 0.4)], [0, 1]),
    "mg_anisotropic_bins": (0, [(1, 1), (-2, 1), (0, 0)], []),
    "mg_agg_nodes": (0, [(50, 50), (-1, 0)], []),
    "mg_replicate_max": (4096, [(100, 100), (-1, 0)], []),
    "asm_packed_codes": (1, [(0, 0), (2, 1)], []),
    "chunk_slots": (256, [(128, 128), (192, 192)], []),
    "contrib_order": (1, [(0, 0), (2, 2)], []),
    "check_every": (50, [(10, 10), (0, 1)], []),
    "keep_host_symbolic": (1, [(0, 0), (1, 1)], []),                              # (false in mfh_ctx; mfh_create switches it on for device -1)
    "reembed": (0, [(1, 1), (0, 0)], []),
    "periodic_ignore_mismatch": (0, [(1, 1), (0, 0)], []),
    "solve_homogeneous": (0, [(1, 1), (0, 0)], []),
    "periodic_ignore_dims": (0, [(5, 5), (15, 7), (8, 0)], []),
    "agg_nodes": (0, [(40, 40), (-2, -2)], []),                                   # plain int cast
    "topology_device": (1, [(0, 0), (1, 1)], []),
    "matrix_storage": (-1, [(0, 0), (1, 1), (-1, -1)], [2, 0.5, -2]),
    "symbolic_device": (1, [(0, 0), (1, 1)], []),
    "sampler_cell_scale": (1.0, [(2.5, 2.5), (0.125, 0.125)], [0, -1, INF, NAN]),
    "xcd_swizzle": (0, [(4, 4), (-1, 0)], []),
    "pcg_graph": (1, [(0, 0), (1, 1)], []),
    "refine": (1, [(0, 0), (1, 1)], []),
    "mf_geometry_from_vertices": (1, [(0, 0), (1, 1)], []),
    "mf_xcd_group": (32, [(8, 8), (-1, 0)], []),
    "vec_grid_cap": (16384, [(2048, 2048), (10, 256)], []),                       # process-wide: put back by the tests that set it
    "dyn_grid_cap": (2048, [(7, 7), (5000, 2048), (0, 1)], []),
    "harmonic_two_pass": (0, [(1, 1), (0, 0)], []),
    "mf_lane_stride": (37, [(5, 5), (0, 1)], []),
    "mf_reorder": (1, [(0, 0), (1, 1)], []),
    "dist_pcg_variant": (1, [(0, 0), (7, 1)], []),
    "dist_profile": (0, [(1, 1), (0, 0)], []),
    "deterministic": (0, [(0, 0)], []),                                           # 1 needs a device: test_deterministic_needs_a_device
    "pcg_variant": (-1, [(1, 1), (0, 0), (-3, -1), (5, 1)], []),
    "mg_batch": (1, [(0, 0), (1, 1)], []),
    "mg_fuse": (1, [(0, 0), (1, 1)], []),
    "mg_dinv_fp32": (1, [(0, 0), (1, 1)], []),
    "auto_stretch_max": (8.0, [(12.5, 12.5), (0.5, 1.0)], []),
    "batch_rhs": (0, [(1, 1), (0, 0)], []),
    "matrix_free_mode": (4, [(3, 3), (1, 1)], []),
    "mf_block_elems": (0, [(192, 192), (0, 0)], []),
    "mf_chunk_rows": (256, [(512, 512), (1, 16), (99999, 4096)], []),
    "mf_chunk_pairs": (2048, [(4096, 4096), (1, 256)], []),
    "matrix_free": (-1, [(0, 0), (7, 1), (-2, -1)], []),
    "tl_rap_agg": (1, [(0, 0), (1, 1)], []),
    "tl_device_aggregates": (1, [(0, 0), (1, 1)], []),
    "tl_probe": (0, [(1, 1), (0, 0)], []),
    "tl_host_inverse": (0, [(1, 1), (0, 0)], []),
}
NAMES = sorted(OPTIONS)


@pytest.fixture
def ctx():
    c = M.Context(-1)
    cap = c.get_option("vec_grid_cap")
    yield c
    c.set_option("vec_grid_cap", cap)
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_default_round_trip_clamp_reject(ctx, name):
    default, pairs, rejected = OPTIONS[name]
    assert ctx.get_option(name) == default
    for value, stored in pairs:
        ctx.set_option(name, value)
        assert ctx.get_option(name) == stored, (value, stored)
    before = ctx.get_option(name)
    for value in rejected:
        with pytest.raises(M.MeshFEMHipError, match=name) as ei:
            ctx.set_option(name, value)
        assert ei.value.code == _lib.ERR_INVALID, value
        assert ctx.get_option(name) == before, value


@pytest.mark.parametrize("name", NAMES)
def test_set_of_get_is_the_identity(ctx, name):
    """a new forced-degree-1 view starts from the values read from its context"""
    for value, stored in [(None, OPTIONS[name][0])] + OPTIONS[name][1]:
        if value is not None:
            ctx.set_option(name, value)
        ctx.set_option(name, ctx.get_option(name))
        assert ctx.get_option(name) == stored, (value, stored)


def test_deterministic_needs_a_device(ctx):
    with pytest.raises(M.MeshFEMHipError) as ei:
        ctx.set_option("deterministic", 1)
    assert ei.value.code == _lib.ERR_HIP
    assert ctx.get_option("deterministic") == 0


def test_unknown_names(ctx):
    for name in ("debug_variant", "mg_step_fine", "matrix-free", "Deterministic", "chunk_slots ", ""):
        for call in (lambda: ctx.set_option(name, 1), lambda: ctx.get_option(name)):
            with pytest.raises(M.MeshFEMHipError, match="unknown option") as ei:
                call()
            assert ei.value.code == _lib.ERR_INVALID, name


def test_the_list_is_the_table():
    """one row per name of the list, and no row that the list does not know"""
    with open(os.path.join(ROOT, "meshfem_amd", "csrc", "mfh_options.cpp")) as f:
        rows = re.findall(r'^\s*\{"([^"]*)",', f.read(), flags=re.M)
    assert len(rows) == len(OPTIONS) == 59
    assert sorted(rows) == NAMES


def test_values_are_finite_doubles(ctx):
    for name in NAMES:
        assert math.isfinite(ctx.get_option(name)), name
