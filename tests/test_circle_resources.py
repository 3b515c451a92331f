"""CPU: resources of the circle transform's kernels, read from the objects the build left under build/obj
(tools/isa_stats.py): no private segment, no static LDS (the tile is dynamic, capped by the route at 64 KB),
work-groups of at most 256 lanes, and registers within the budget of four waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
# object -> the kernels it must hold (substrings of the mangled names)
OBJECTS = {
    "m31__circle_k_circle.hip__SPPARK_CIRCLE_INV=0.o": ("13k_circle_passILb0E",),
    "m31__circle_k_circle.hip__SPPARK_CIRCLE_INV=1.o": ("13k_circle_passILb1E",),
    "m31__api_circle_api.hip.o": ("15k_circle_points", "18k_circle_inv_table", "8k_bitrevI", "14k_bitrev_tiledI", "18k_bitrev_tiled_vecI"),
}


@pytest.mark.parametrize("obj", sorted(OBJECTS))
def test_circle_kernels_resources(libs, obj):
    import isa_stats
    path = os.path.join(OBJ, obj)
    if not os.path.exists(path):
        pytest.skip("%s not built here" % obj)          # (a tree whose libraries arrived prebuilt, without objects)
    kernels = {sym: md for sym, md in isa_stats.metadata(isa_stats.code_object(path)).items() if "vgpr_count" in md}
    for tag in OBJECTS[obj]:
        assert any(tag in sym for sym in kernels), (obj, tag, sorted(kernels))
    assert len(kernels) == len(OBJECTS[obj]), sorted(kernels)
    for sym, md in kernels.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, sym
        assert int(md.get("group_segment_fixed_size") or 0) <= 65536, sym
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, sym
        # a work-group holds up to 34 KB of LDS: four of them per CU, four waves per SIMD, 128 registers each
        assert int(md.get("vgpr_count") or 0) + int(md.get("agpr_count") or 0) <= 128, sym
        assert "k_vec" not in sym
