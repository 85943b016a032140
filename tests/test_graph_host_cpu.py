"""CPU side of the graph unit's host logic (csrc/graph_host.hpp): the seed list, the connectivity repair and CSR assembly of the build, the
traversal's launch plan with its refusals and the tail merge's arithmetic pass their stand-alone check (tests/native/graph_host_check.cpp) under
the address and undefined-behaviour sanitizers; the seed list the header computes for the golden graph is the oracle's PrepareInitIds; the header
holds no device type."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("graph_host") / "graph_host_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "native", "graph_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    return subprocess.run([exe] + list(args), capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))


def test_host_logic_is_clean_under_address_and_ub_sanitizers(check_exe):
    r = run(check_exe)
    assert r.returncode == 0 and "graph_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_seed_list_equals_the_oracles_prepare_init_ids(oracle, check_exe, tmp_path):
    z = np.load(os.path.join(G, "graph2000x32.npz"))
    off, nbr, nav = z["off"].astype(np.int64), z["nbr"].astype(np.int64), int(z["nav"])
    path = str(tmp_path / "graph.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(off) - 1, nav], np.int64).tobytes() + off.tobytes() + nbr.tobytes())
    for L in (1, 32, 500, 2000):
        r = run(check_exe, "seeds", path, str(L))
        assert r.returncode == 0, (L, r.stdout[-2000:], r.stderr[-3000:])
        got = np.array(r.stdout.split(), np.int64)
        want = oracle.prepare_init_ids(off, nbr, nav, L)
        assert got.shape == (L,) and np.array_equal(got, want), L


def test_evaluation_log_sizes_of_the_filtered_cases_are_the_headers(oracle, check_exe):
    """tests/filtered_walk_ref.py restates the size of the filtered traversal's evaluation log (first_log) to choose its repeat case on the CPU:
    for every case of its list, and for the repeat case's second attempt, the header's trv_launch gives the same number."""
    import filtered_walk_ref as fr
    seen = set()
    for c in fr.all_cases():
        key = (c["n"], c["nq"], min(c["L"], c["n"]))
        if key in seen:
            continue
        seen.add(key)
        r = run(check_exe, "ecap", str(key[0]), str(key[1]), str(key[2]), "0")
        assert r.returncode == 0 and int(r.stdout) == fr.first_log(key[0], key[2]), (key, r.stdout, r.stderr[-2000:])
    g = fr.cases_g()[0]
    init, walks = fr.logged_walks(oracle, g)
    need = fr.repeat_log(g["n"], max(w[2] for w in walks))
    assert need == fr.REPEAT_SECOND_LOG       # (the figure pinned in graph_host_check.cpp repeat_log())
    r = run(check_exe, "ecap", str(g["n"]), str(g["nq"]), str(g["L"]), str(need))
    assert r.returncode == 0 and int(r.stdout) == need, (r.stdout, r.stderr[-2000:])


def test_the_header_holds_no_device_type():
    src = open(os.path.join(ROOT, "vectordb_amd", "csrc", "graph_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).replace("__HIPCC__", "").lower()
    # ... and the units that used to carry their own copies go through it
    trv = open(os.path.join(ROOT, "vectordb_amd", "csrc", "traverse.hip")).read()
    bld = open(os.path.join(ROOT, "vectordb_amd", "csrc", "graph_build.hip")).read()
    assert "seed_list(" in trv and bld.count("seed_list(") == 2 and "repair_orphans(" in bld and "graph_csr(" in bld
    assert "trv_queues(" in trv and "trv_launch(" in trv and "tail_plan(" in trv
