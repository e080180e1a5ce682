"""Objects without a GPU (include/jefferson.h: "objects"): the declarations stand in the headers, the library
exports them, the binding binds them, and every one of them refuses a null engine."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

PUBLIC = ["jf_engine_set_objects", "jf_num_objects", "jf_source_set_object", "jf_source_object", "jf_object_set_world",
          "jf_object_get_world", "jf_process_batch_objects", "jf_batch_upload_objects"]
DEBUG = ["jf_debug_pose_objects_device"]


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(jf_[a-z0-9_]+)\s*\(", src))


def test_objects_are_declared_exported_and_bound(jf):
    assert set(PUBLIC) <= _declared("jefferson.h") and set(DEBUG) <= _declared("jefferson_debug.h")
    text = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    assert re.search(r"#define\s+JF_MAX_OBJECTS\s+65536\b", text) and "cudaPart.cu:198-199" in text
    L = ctypes.CDLL(jf.LIB_PATH)
    assert not [n for n in PUBLIC + DEBUG if not hasattr(L, n)]
    assert set(PUBLIC + DEBUG) <= set(jf.exported_symbols())
    for name in ("set_objects", "n_objects", "set_object", "object_of", "set_object_world", "object_world",
                 "process_batch_objects", "upload_objects", "pose_objects_device"):
        assert hasattr(jf.Engine, name), name


def test_objects_refuse_a_null_engine(jf):
    L, fp = jf.lib(), jf._fp
    o, q, mix, rec = np.zeros((1, 1, 3), np.float32), np.float32([[[0, 0, 0, 1, 0, 0, 0]]]), np.zeros(512, np.float32), np.zeros(5, np.float32)
    m = np.zeros(1, np.int32)
    assert L.jf_engine_set_objects(None, 1) == jf.JF_ERR_ARG
    assert L.jf_num_objects(None) == jf.JF_ERR_ARG and L.jf_num_objects(None) < 0
    assert L.jf_source_set_object(None, 0, 0) == jf.JF_ERR_ARG
    assert L.jf_source_object(None, 0) == jf.JF_ERR_ARG and L.jf_source_object(None, 0) < 0
    assert L.jf_object_set_world(None, 0, 0.0, 0.0, -1.0) == jf.JF_ERR_ARG
    assert L.jf_object_get_world(None, 0, fp(np.zeros(3, np.float32))) == jf.JF_ERR_ARG
    assert L.jf_process_batch_objects(None, 1, None, fp(o), fp(q), fp(mix)) == jf.JF_ERR_ARG
    assert L.jf_batch_upload_objects(None, 1, fp(o), fp(q)) == jf.JF_ERR_ARG
    assert L.jf_debug_pose_objects_device(None, 1, 1, 1, 1, None, jf._ip(m), fp(o), fp(q), fp(rec)) == jf.JF_ERR_ARG
    # ... and null everything
    assert L.jf_process_batch_objects(None, 0, None, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_batch_upload_objects(None, 0, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_pose_objects_device(None, 0, 0, 0, 0, None, None, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_object_get_world(None, 0, None) == jf.JF_ERR_ARG
