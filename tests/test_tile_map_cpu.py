"""The block -> tile arithmetic of every GEMM launch (cqa-crct_amd/csrc/tile_map.h) on its own: the header includes nothing from HIP,
so tests/tile_map_check.cpp is built with the host compiler and run here -- no GPU, no Python extension.  The kernels of gemm.hip call
the same definitions, so a tile that this walk finds skipped, visited twice or placed past a buffer is one the GPU would compute wrongly
(or write into a neighbour's memory) at that shape."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["128x128", "64x64", "64x128", "128x64", "256x128"]      # every tile shape of k_configs (gemm.hip)
SINGLE = ["grid_is_8_rectangles",             # gm * gn == 8, rm / rn their ceilings, grid == 8 * rm * rn
          "true_count_is_tile_count",         # over bid in [0, grid): map_tile is true tiles_m * tiles_n times
          "every_tile_exactly_once",          # ... and yields every (tm, tn) in range once
          "every_other_block_false"]          # the padding blocks, and whatever lies behind the grid
SPLITK = ["every_tile_slice_exactly_once",    # over grid * S blocks, S = 2 .. 8
          "slices_of_a_tile_share_an_xcd",    # equal bid & 7
          "ticket_inside_ticket_array",       # tile_lin < crct_gemm_splitk_tickets(M, N)
          "slabs_inside_workspace",           # (tile_lin + 1) * S * BM * BN <= crct_gemm_splitk_ws_elems(M, N, S)
          "no_workspace_unsplit"]
GROUP = ["edge_groups_present",               # all problems one tile; fewer than 8 tiles in all; a total that is no multiple of 8
         "problems_begin_on_xcd_0",           # tile_begin[i] % 8 == 0
         "default_every_tile_exactly_once",   # every (problem, tm, tn) once over [0, tile_begin[n])
         "concat_total_is_8_per_xcd",
         "concat_every_tile_exactly_once",
         "concat_xcd_owns_one_run_of_the_list",   # the blocks of XCD x yield consecutive entries of the concatenated tile list
         "concat_padding_blocks_false"]
GRID = ["group_grid_between_1_and_total",
        "group_grid_multiple_of_8_or_total",
        "group_grid_target_keeps_the_rounds",              # ceil(total / grid) <= ceil(total / target)
        "group_grid_walk_stays_on_one_xcd",                # grid % 8 == 0: b, b + grid, ... keep b & 7
        "group_grid_cap_overrides_target",
        "group_grid_other_kinds_ignore_target_obey_cap"]   # forward, data-gradient and fp8 groups
CASES = (["single_%s_%s" % (s, c) for s in SHAPES for c in SINGLE] + ["splitk_%s_%s" % (s, c) for s in ("128x128", "128x64") for c in SPLITK] +
         ["group_%s_%s" % (s, c) for s in ("128x128", "128x64") for c in GROUP] + GRID)
HEADER = os.path.join(ROOT, "cqa-crct_amd", "csrc", "tile_map.h")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tile_map") / "tile_map_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cqa-crct_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "tile_map_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return run.returncode, dict(line.split() for line in run.stdout.splitlines()), run.stderr


def test_header_includes_nothing_from_hip():
    with open(HEADER) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(inc in ("<stdint.h>", '"crct_hip.h"') for inc in includes), includes      # crct_hip.h is the plain-C interface
    with open(os.path.join(ROOT, "include", "crct_hip.h")) as f:
        assert all(line.split()[1] in ("<stddef.h>", "<stdint.h>") for line in f if line.startswith("#include"))


def test_gemm_hip_runs_the_header_definitions():
    """One definition: gemm.hip includes the header and keeps no copy of the arithmetic of its own."""
    with open(os.path.join(ROOT, "cqa-crct_amd", "csrc", "gemm.hip")) as f:
        src = f.read()
    assert '#include "tile_map.h"' in src
    for name in ("map_tile", "map_splitk", "group_pick", "group_add", "group_concat", "group_grid", "group_cap", "group_total", "make_tile_map",
                 "splitk_ws_elems", "splitk_tickets"):
        assert "crct::" + name in src, name
    for own in ("bool map_tile(", "bool group_pick(", "void group_concat(", "int group_grid(", "struct TileMap {", "(M + 127) / 128"):
        assert own not in src, own


@pytest.mark.parametrize("case", CASES)
def test_tile_placement(report, case):
    status, lines, err = report
    assert lines.get(case) == "ok", (case, err)


def test_every_case_ran_and_passed(report):
    status, lines, err = report
    assert status == 0 and sorted(lines) == sorted(CASES), (status, lines, err)
