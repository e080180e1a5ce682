"""Live input at the boundary, without a GPU: the entry points of include/jefferson.h that feed sources block by block
(jf_source_set_live, the *_in calls -- the `input` argument the reference's paCallback drops, Audio.cu:164-175) are declared,
exported and bound; each refuses null or zero arguments with JF_ERR_ARG and without a fault; jf_render offers --live."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

LIVE = ["jf_source_set_live", "jf_num_live_sources", "jf_submit_block_in", "jf_process_block_in", "jf_callback_in",
        "jf_process_batch_in"]


def _header():
    return open(os.path.join(ROOT, "include", "jefferson.h")).read()


def test_live_entry_points_are_declared_and_exported(jf):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = re.findall(r"\b(jf_[a-z0-9_]+)\s*\(", src)
    L = C.CDLL(jf.LIB_PATH)
    for name in LIVE:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in jf.exported_symbols(), name


def test_live_declarations_cite_the_input_the_reference_drops():
    """the comments over the new declarations name paCallback's input argument and copyIncomingBlock"""
    src = _header()
    for name in LIVE:
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "Audio.cu:164-175" in comment, name
    assert "GPUSoundSource.cu:481-513" in src[src.index("LIVE INPUT"):src.index("jf_source_set_live(jf_engine")]


def test_live_entry_points_refuse_null_arguments(jf):
    """a null engine, null buffers, zero counts: JF_ERR_ARG, no fault (no GPU is touched: a null handle is refused first)"""
    L = jf.lib()
    out = (C.c_float * 512)()
    pos = (C.c_float * 5)()
    assert L.jf_source_set_live(None, 0, 1) == jf.JF_ERR_ARG
    assert L.jf_source_set_live(None, -1, 0) == jf.JF_ERR_ARG
    assert L.jf_num_live_sources(None) == jf.JF_ERR_ARG
    assert L.jf_submit_block_in(None, None) == jf.JF_ERR_ARG
    assert L.jf_submit_block_in(None, out) == jf.JF_ERR_ARG
    assert L.jf_process_block_in(None, None, None) == jf.JF_ERR_ARG
    assert L.jf_process_block_in(None, out, out) == jf.JF_ERR_ARG
    assert L.jf_callback_in(None, None, None) == jf.JF_ERR_ARG
    assert L.jf_callback_in(None, out, out) == jf.JF_ERR_ARG
    assert L.jf_process_batch_in(None, 0, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_process_batch_in(None, 1, out, pos, out) == jf.JF_ERR_ARG
    assert L.jf_debug_reverb_ahead_pending(None) == jf.JF_ERR_ARG
    # PortAudio's trampoline with an input buffer and no engine: silence, paContinue
    buf = (C.c_float * 512)(*([1.0] * 512))
    assert L.jf_pa_callback(out, buf, 256, None, 0, None) == 0
    assert not any(buf)


def test_engine_binding_offers_the_live_forms(jf):
    import inspect
    E = jf.Engine
    assert hasattr(E, "set_live") and hasattr(E, "n_live")
    for name in ("process_block", "submit_block", "callback"):
        assert "inp" in inspect.signature(getattr(E, name)).parameters, name
    assert list(inspect.signature(E.process_batch).parameters)[1:] == ["pos", "inp"]


def test_jf_render_names_live():
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_render")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and "--live" in r.stderr.decode()
