"""CPU tests of the drop-in boundary: the shared library loads, exports every symbol
include/dspmap.h declares, host-only entry points work, and compute entry points FAIL LOUDLY
without a GPU (there is no CPU fallback in the product)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dspmap_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_all_exported_and_bound(dsp):
    names = declared_symbols()
    assert len(names) >= 45
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (dspmap_[a-z_0-9]+)", out))
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    assert sorted(dsp.capi.SIGNATURES) == names  # the ctypes binding covers exactly the header
    for n in names:
        assert getattr(lib, n) is not None


def test_library_has_gfx950_code_object(dsp):
    blob = open(dsp.capi.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for k in (b"k_predict", b"k_place", b"k_ck_partial", b"k_weight", b"k_birth_insert", b"k_resample"):
        assert k in blob, k


def test_host_only_entry_points(dsp, orc):
    m = dsp.DSPMap(dsp.make_config(ppv=24))
    o = orc.Oracle(orc.make_config(ppv=24))
    assert (m.V, m.slots, m.NP, m.capp) == (o.V, o.slots, o.NP, o.capp)
    idx = C.c_int()
    x, y, z = C.c_float(), C.c_float(), C.c_float()
    rng = np.random.default_rng(0)
    for _ in range(2000):
        p = rng.uniform(-5.2, 5.2, 3).astype(np.float32)
        ok, i = m.getPointVoxelsIndexPublic(float(p[0]), float(p[1]), float(p[2]))
        ok_o = o.L.dspo_voxel_index(o.h, float(p[0]), float(p[1]), float(p[2]), C.byref(idx))
        assert ok == ok_o and (not ok or i == idx.value)
    for v in (0, 1, 66, 4356, 174239):
        o.L.dspo_voxel_center(o.h, v, C.byref(x), C.byref(y), C.byref(z))
        assert m.getVoxelPositionFromIndexPublic(v) == (x.value, y.value, z.value)
    assert m.L.dspmap_get_param(m.h, dsp.capi.P_OBSERVATION_STDDEV) == pytest.approx(0.1)
    assert m.L.dspmap_set_param(m.h, 999, 1.0) < 0
    assert b"unknown parameter" in m.L.dspmap_last_error(m.h)
    m.close(); o.close()


def test_create_rejects_bad_config(dsp):
    L = dsp.load_library()
    bad = dsp.make_config(nx=0)
    assert not L.dspmap_create(C.byref(bad))
    bad = dsp.make_config(ppv=65)
    assert not L.dspmap_create(C.byref(bad))
    bad = dsp.make_config(z_lo=30, z_hi=50)
    assert not L.dspmap_create(C.byref(bad))
    # the immediate neighbours outside the configuration space (tests/config_edges.py): 65 particles per voxel, 129 slots, 17 horizons,
    # 130 / 98 pyramids per axis at 1 degree, 2^31 cells -- and the nearest configuration inside is accepted
    from tests import config_edges as E
    assert sorted(E.OUTSIDE) == ["cells_2p31", "fov_h65", "fov_v49", "ppv65", "slots129", "t17"]
    for name in E.OUTSIDE:
        assert not L.dspmap_create(C.byref(E.outside_config(dsp.make_config, name))), name
    for kw in (dict(ppv=64), dict(ppv=32, safe_factor=4), dict(pred_times=E.T16), dict(angle=1, half_fov_h=64, half_fov_v=48),
               dict(nx=1024, ny=1024, nz=1023, ppv=1)):
        h = L.dspmap_create(C.byref(dsp.make_config(**dict(E.SMALL, **kw))))
        assert h, kw
        L.dspmap_destroy(h)


def test_compute_fails_loudly_without_gpu(dsp):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    m = dsp.DSPMap()
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(dsp.capi.DSPMapError, match="no HIP device"):
        m.update(pts, (0, 0, 0), 0.0, (1, 0, 0, 0))
    with pytest.raises(dsp.capi.DSPMapError):
        m.getOccupancyMap(0.2)
    m.close()


def test_product_never_imports_oracle():
    """the product package must not reference oracle/ (a CPU fallback would void parity claims)"""
    pkg = os.path.join(ROOT, "dsp-map_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                t = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_py" not in t and "dsp_oracle" not in t and "dspo_" not in t, f


def test_dropin_header_compiles_without_ros(dsp):
    """include/dsp_dynamic.h (ours) offers the reference's DSPMap surface; the ROS-free twin of
    src/map_sim_example.cpp must compile and link against libdspmap_hip.so"""
    exe = os.path.join(ROOT, "examples", "map_example")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "map_example.cpp"),
                           "-L" + os.path.join(ROOT, "dsp-map_amd", "lib"), "-ldspmap_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "dsp-map_amd", "lib"), "-o", exe])
    # the reference's two other headers as macro sets in front of the same header
    for macros in (["-DMAP_LENGTH_VOXEL_NUM=50", "-DMAP_WIDTH_VOXEL_NUM=50", "-DMAP_HEIGHT_VOXEL_NUM=30", "-DVOXEL_RESOLUTION=0.2",
                    "-DANGLE_RESOLUTION=1", "-DPYRAMID_NEIGHBOR_N=2", "-DMAX_PARTICLE_NUM_VOXEL=30", "-DDSPMAP_HALF_FOV_V=27",
                    "-DDSPMAP_OCCLUSION_MARGIN=VOXEL_RESOLUTION"],
                   ["-DMAP_LENGTH_VOXEL_NUM=50", "-DMAP_WIDTH_VOXEL_NUM=50", "-DMAP_HEIGHT_VOXEL_NUM=30", "-DVOXEL_RESOLUTION=0.2",
                    "-DMAX_PARTICLE_NUM_VOXEL=10", "-DDSPMAP_STATIC_MODEL=1", "-DDSPMAP_SAFE_PARTICLE_FACTOR=5",
                    "-DPREDICTION_TIMES=1", "-DDSPMAP_HALF_FOV_V=27", "-DDSPMAP_OCCLUSION_MARGIN=VOXEL_RESOLUTION"],
                   ["-DDSPMAP_WORLD=1"]):   # the sharded build of the same class (C++ RCCL driver)
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + macros +
                              [os.path.join(ROOT, "examples", "map_example.cpp")])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for member in ("int update(int point_cloud_num, int size_of_one_point, float* point_cloud_ptr",
                   "void setPredictionVariance(float p_stddev, float v_stddev)", "void setObservationStdDev(",
                   "void setNewBornParticleWeight(", "void setNewBornParticleNumberofEachPoint(",
                   "void setParticleRecordFlag(", "static void setOriginalVoxelFilterResolution(",
                   "void getOccupancyMap(int& obstacles_num", "void getOccupancyMapWithFutureStatus(int& obstacles_num",
                   "void clearOccupancyMapPrediction()", "void getKMClusterResult(",
                   "void mapAddNewBornParticlesByObservation()", "static float generateRandomFloat(",
                   "void getVoxelPositionFromIndexPublic(", "int getPointVoxelsIndexPublic(", "void getFutureStatus("):
        assert member in hdr, member


def test_parameter_ids_of_the_binding_match_the_header(dsp):
    """every DSPMAP_P_* enumerator of include/dspmap.h has a P_* constant of the same value in the ctypes binding (a new
    parameter that is added to one side only would silently address another one), and the scheduling knobs are plain
    host state: settable and readable without a device"""
    text = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ids = dict((k, int(v)) for k, v in re.findall(r"\bDSPMAP_P_([A-Z_0-9]+)\s*=\s*(\d+)", text))
    assert len(ids) >= 19 and len(set(ids.values())) == len(ids)
    for name, val in ids.items():
        assert getattr(dsp.capi, "P_" + name) == val, name
    m = dsp.DSPMap(dsp.make_config(ppv=24))
    for key in (dsp.capi.P_SPARSE_SWEEP, dsp.capi.P_ROLLOUT_INLINE):
        for v in (1, 0, -1):
            assert m.L.dspmap_set_param(m.h, key, float(v)) == 1
    m.close()


def test_pair_path_readbacks_are_declared_bound_and_check_their_arguments(dsp):
    """dspmap_debug_pair_items / dspmap_debug_weight_variant (which pair-kernel path the last weight update took): in the header, in the
    binding, NULL handles and NULL outputs are argument errors, and a handle that has not run a weight update reports no variant"""
    assert {"dspmap_debug_pair_items", "dspmap_debug_weight_variant"} <= set(declared_symbols()) & set(dsp.capi.SIGNATURES)
    L = dsp.load_library()
    out = (C.c_int * 3)()
    assert L.dspmap_debug_pair_items(None, out) == -1 and L.dspmap_debug_weight_variant(None) == -1
    m = dsp.DSPMap(dsp.make_config(ppv=24))
    assert m.weight_variant() is None
    import torch
    if torch.cuda.is_available():
        assert L.dspmap_debug_pair_items(m.h, None) == -1
    else:
        assert L.dspmap_debug_pair_items(m.h, out) < 0 and b"no HIP device" in L.dspmap_last_error(m.h)
    m.close()


def test_rendezvous_file_is_matched_by_its_nonce_string(dsp, tmp_path, monkeypatch):
    """dspmap_mgpu_comm_init_from_env (the drop-in class's sharded start-up, -DDSPMAP_WORLD): a rank != 0 accepts exactly the record
    whose nonce STRING is this launch's -- whatever follows the string's NUL in the 120-byte field (rank 0's stack residue before
    the fix; zeros; anything) does not count; another launch's nonce, a wrong magic or a short file are refused"""
    L = dsp.load_library()
    monkeypatch.setenv("DSPMAP_RDZV_NONCE", "run-42")
    path = str(tmp_path / "rdzv")
    uid = bytes(range(128))
    out = C.create_string_buffer(128)
    # what rank 0 publishes is what the others wait for
    assert L.dspmap_debug_rdzv_publish(path.encode(), uid) == 1
    assert L.dspmap_debug_rdzv_wait(path.encode(), 50, out) == 1 and out.raw == uid
    nonce = ("run-42:%d" % os.getppid()).encode()
    assert open(path, "rb").read()[8:8 + len(nonce) + 1] == nonce + b"\0"
    # a hand-made record: correct string, garbage behind its NUL
    rec = b"DSPRDZV1" + nonce + b"\0" + b"\xa5" * (120 - len(nonce) - 1) + uid
    open(path, "wb").write(rec)
    out = C.create_string_buffer(128)
    assert L.dspmap_debug_rdzv_wait(path.encode(), 50, out) == 1 and out.raw == uid
    # ... zero-padded
    open(path, "wb").write(b"DSPRDZV1" + nonce.ljust(120, b"\0") + uid)
    assert L.dspmap_debug_rdzv_wait(path.encode(), 50, out) == 1
    # refused: another launch's nonce (also one that merely starts like ours), wrong magic, truncated file, no file
    for bad in (b"DSPRDZV1" + (nonce + b"7").ljust(120, b"\0") + uid,
                b"DSPRDZV1" + b"run-41:1".ljust(120, b"\0") + uid,
                b"DSPRDZV0" + nonce.ljust(120, b"\0") + uid,
                (b"DSPRDZV1" + nonce.ljust(120, b"\0") + uid)[:200]):
        open(path, "wb").write(bad)
        assert L.dspmap_debug_rdzv_wait(path.encode(), 30, out) == 0
    os.unlink(path)
    assert L.dspmap_debug_rdzv_wait(path.encode(), 30, out) == 0
    monkeypatch.setenv("DSPMAP_RDZV_NONCE", "run-43")                      # a later launch does not take the old file
    open(path, "wb").write(b"DSPRDZV1" + nonce.ljust(120, b"\0") + uid)
    assert L.dspmap_debug_rdzv_wait(path.encode(), 30, out) == 0


def test_rebuild_decision_follows_the_source_hash_not_the_clock(dsp, tmp_path, monkeypatch):
    """build_ext.needs_build() compares a sha256 of the sources / headers / flags with the one stored next to the .so when it was
    built: a tree that arrives by a `gpurun` push (fresh mtimes everywhere) is not rebuilt needlessly and -- the dangerous
    direction -- a .so that is NEWER than edited sources is not trusted."""
    import build_ext
    assert os.path.exists(build_ext.LIB) and os.path.exists(build_ext.STAMP)
    assert open(build_ext.STAMP).read().strip() == build_ext.source_hash() and not build_ext.needs_build()
    os.utime(os.path.join(build_ext.CSRC, build_ext.SOURCES[0]))          # a newer clock on a source changes nothing
    assert not build_ext.needs_build()
    monkeypatch.setattr(build_ext, "FLAGS", build_ext.FLAGS + ["-DX=1"])   # other flags = another library
    assert build_ext.needs_build()
    monkeypatch.undo()
    monkeypatch.setattr(build_ext, "STAMP", str(tmp_path / "missing"))     # no record of what the .so was built from
    assert build_ext.needs_build()


def _reference_caller_source(surface, with_eigen):
    """a translation unit that uses the DSPMap surface the way the reference's node does (tests/golden/reference_caller_surface.json):
    a global map built during static initialisation, every recorded member called with arguments of the recorded types, the
    configuration macros as constant expressions and array bounds, the std names unqualified; with_eigen: also the globals of Eigen
    types, which the caller gets through the header alone"""
    src = ["#include <%s>" % h for h in surface["own_includes"]] + ['#include "%s"' % surface["header"], ""]
    obj = surface["global_object"]
    src += ["DSPMap %s;" % obj, ""]
    src += ["static %s std_name_%d;" % (n, i) for i, (n, kind) in enumerate(surface["unqualified_std_names"].items()) if kind == "type"]
    if with_eigen:
        src += ["static %s eigen_global_%d;" % (n, i) for i, n in enumerate(surface["eigen_globals"])]
    src += ["static_assert(%s > 0, \"%s\");" % (c, c) for c in surface["int_constants"]]
    src += ["static float array_%d%s;" % (i, "".join("[%s]" % b for b in dims)) for i, dims in enumerate(surface["static_array_bounds"])]
    src += ["", "int main() {"]
    src += ["    const float constant_%d = %s * %s / 2;" % (i, c, surface["int_constants"][0]) for i, c in enumerate(surface["float_constants"])]
    src += ["    std::cout << constant_%d << %s;" % (i, n) for i in range(len(surface["float_constants"]))
            for n, kind in surface["unqualified_std_names"].items() if kind == "manipulator"]
    for i, call in enumerate(surface["calls"]):
        names = []
        for j, t in enumerate(call["args"]):
            names.append("a%d_%d" % (i, j))
            src.append("    %s %s{};" % (t.rstrip("&"), names[-1]))
        expr = "%s%s(%s)" % ("DSPMap::" if call["static"] else obj + ".", call["member"], ", ".join(names))
        src.append("    if (!%s) return 1;" % expr if call["result_as_condition"] else "    %s;" % expr)
    src += ["    return 0;", "}", ""]
    return "\n".join(src)


def test_reference_caller_type_checks_against_the_drop_in_header(tmp_path):
    """include/dsp_dynamic.h offers what the reference's node (its src/map_sim_example.cpp) needs to compile against it unchanged:
    g++ -fsyntax-only on a caller generated from the recorded surface (tests/golden/reference_caller_surface.json), once with the
    header's own minimal pcl containers and once with PCL and Eigen installations in front of it (declaration-only stubs in a temp
    dir), where the Eigen types of the node's globals must arrive through the header's include"""
    import json
    surface = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_caller_surface.json")))
    assert len(surface["calls"]) >= 9 and surface["eigen_globals"]
    pcl = tmp_path / "stubs" / "pcl"
    pcl.mkdir(parents=True)
    (pcl / "point_types.h").write_text(
        "#pragma once\n#include <vector>\n#include <memory>\n#include <cstddef>\nnamespace pcl {\nstruct PointXYZ { float x, y, z; };\n"
        "struct PointXYZINormal { float x, y, z, intensity, normal_x, normal_y, normal_z; };\n"
        "template <class T> struct PointCloud { typedef std::shared_ptr<PointCloud<T> > Ptr; std::vector<T> points; unsigned width, height;\n"
        "    void push_back(const T&); void clear(); size_t size() const; bool empty() const; T& operator[](size_t); };\n}\n")
    (pcl / "point_cloud.h").write_text("#include <pcl/point_types.h>\n")
    eigen = tmp_path / "stubs" / "Eigen"
    eigen.mkdir()
    (eigen / "Eigen").write_text("#pragma once\nnamespace Eigen {\nstruct Vector3d { double x() const; double y() const; double z() const; };\n"
                                 "struct Quaternionf { float w() const; float x() const; float y() const; float z() const; };\n}\n")
    flags = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-sign-compare",
             "-Wno-unused-function", "-I" + os.path.join(ROOT, "include")]
    for with_libs in (False, True):
        caller = tmp_path / ("caller_%d.cpp" % with_libs)
        caller.write_text(_reference_caller_source(surface, with_eigen=with_libs))
        extra = ["-I" + str(tmp_path / "stubs")] if with_libs else []
        r = subprocess.run(flags + extra + [str(caller)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, caller.read_text() + r.stderr[-4000:]
