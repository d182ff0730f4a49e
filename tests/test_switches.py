"""CPU: havatar_amd/switches.py -- the truth rule of every switch as the expressions it replaced had it (written out below as literals), reads that
happen at the call against the three that happen at import, no other reader of a HAVATAR_* / HAV_* variable in the package, and the table against the
accessor calls, the library's getenv calls and README's "Switches" table."""
import ast
import glob
import os
import re

import pytest

from havatar_amd import switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "havatar_amd")

# what an unset variable and the values "0", "1", "", "2", "off" select
VALUES = (None, "0", "1", "", "2", "off")
ON_EXPECT = (True, False, True, True, True, True)                 # os.environ.get(NAME, "1") != "0"
OFF_EXPECT = (False, False, True, False, False, False)            # os.environ.get(NAME, "0") == "1"

ON = ("HAVATAR_FINE_CACHE", "HAVATAR_LPIPS", "HAVATAR_METRICS", "HAVATAR_CONV_AUTOSCALE", "HAVATAR_S2_WGRAD", "HAVATAR_CONV_BWD", "HAVATAR_CONV_WGRAD",
      "HAVATAR_FUSED_BLOCK", "HAVATAR_S2_DGRAD", "HAVATAR_FUSED_UPBLOCK", "HAVATAR_CONV3D_SMALL", "HAVATAR_S2_LOSS", "HAVATAR_HIP_TRAIN",
      "HAVATAR_FUSED_CONV", "HAVATAR_EQUAL_LINEAR", "HAVATAR_FUSED_UPCONV", "HAVATAR_CONV_S2", "HAVATAR_S2_INFER", "HAVATAR_S2_TRAIN",
      "HAVATAR_FUSED_HAAR", "HAVATAR_FUSED_TORGB", "HAVATAR_STYLE_BATCH", "HAVATAR_STYLE_MLP", "HAVATAR_FIELD_MLP", "HAVATAR_ENC_STREAMS",
      "HAVATAR_HIP_GATHER", "HAVATAR_TRAIN_GRAPH", "HAVATAR_FUSED_ADAM", "HAVATAR_DET_MIOPEN", "HAVATAR_DET_ATEN", "HAVATAR_DEVICE_RAYS", "HAVATAR_GRAPH")
OFF = ("HAVATAR_REQUIRE_TESTED_HIPCC", "HAVATAR_GRAPH_SHAPE", "HAVATAR_DEBUG_SYNC", "HAVATAR_DETERMINISTIC", "HAVATAR_COMPOSITE_LONG",
       "HAVATAR_HAAR_TRAIN", "HAVATAR_CONV_1X1", "HAVATAR_FIELD_ROWS")
# (name, value, what the accessor returns); the comment is what the caller makes of it
CHOICE = (("HAVATAR_TRAIN_MLP", None, "bf16"), ("HAVATAR_TRAIN_MLP", "bf16", "bf16"),          # == "bf16": the bf16 route
          ("HAVATAR_TRAIN_MLP", "torch", "torch"), ("HAVATAR_TRAIN_MLP", "BF16", "BF16"),       # anything else: torch's
          ("HAVATAR_RESAMPLE", None, "hip"), ("HAVATAR_RESAMPLE", "aten", "aten"), ("HAVATAR_RESAMPLE", "junk", "junk"),          # != "aten": the kernel
          ("HAVATAR_S2_TRAIN_FWD", None, "kernel"), ("HAVATAR_S2_TRAIN_FWD", "aten", "aten"), ("HAVATAR_S2_TRAIN_FWD", "junk", "junk"),   # == "aten"
          ("HAVATAR_CONV3D", None, ""), ("HAVATAR_CONV3D", "hip", "hip"), ("HAVATAR_CONV3D", "1", "1"),          # == "hip"
          ("HAVATAR_DECODER", None, ""), ("HAVATAR_DECODER", "hip", "hip"), ("HAVATAR_DECODER", "1", "1"),       # == "hip"
          ("HAVATAR_GRAPH_CAPTURE_STREAM", None, ""), ("HAVATAR_GRAPH_CAPTURE_STREAM", "own", "own"), ("HAVATAR_GRAPH_CAPTURE_STREAM", "1", "1"),
          ("HAVATAR_MLP", None, "mx"), ("HAVATAR_MLP", "f32", "f32"), ("HAVATAR_MLP", "junk", "junk"),
          ("HAV_MARCH", None, ""), ("HAV_MARCH", "pair", "pair"), ("HAV_FINE", None, ""), ("HAV_FINE", "cache", "cache"),
          ("HAVATAR_NAN_TRACE", None, ""), ("HAVATAR_NAN_TRACE", "", ""), ("HAVATAR_NAN_TRACE", "2", "2"))
INT_DEFAULTS = {"HAVATAR_TRAIN_CHUNK_RAYS": 32768, "HAVATAR_PRETRAIN_WC": 3000, "HAVATAR_FRAME_BATCH": 1, "HAVATAR_PNG_THREADS": 12, "HAVATAR_WORKERS": None}
LIBRARY = ("HAVATAR_UFD", "HAVATAR_UFD_SEG", "HAVATAR_UFD_DOWN2", "HAVATAR_CONV_KERNEL", "HAVATAR_CONV_KSPLIT_CUS", "HAVATAR_FIELD_BWD",
           "HAVATAR_COMPOSITE_BWD", "HAV_ABLATE", "HAV_STAGGER")
ACCESSORS = ("on", "off", "choice", "integer", "path")


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _kind(kind):
    return sorted(n for n, row in switches.TABLE.items() if row[0] == kind)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. truth table
# ------------------------------------------------------------------------------------------------------------------------------------
def test_every_row_is_of_the_kind_the_replaced_expression_had():
    assert _kind("on") == sorted(ON) and _kind("off") == sorted(OFF)
    assert _kind("choice") == sorted({n for n, _, _ in CHOICE}) and _kind("int") == sorted(INT_DEFAULTS)
    assert _kind("path") == ["HAVATAR_LIB"] and _kind("library") == sorted(LIBRARY)
    assert len(switches.TABLE) == len(ON) + len(OFF) + len({n for n, _, _ in CHOICE}) + len(INT_DEFAULTS) + 1 + len(LIBRARY)
    for name, (kind, default, read) in switches.TABLE.items():
        assert read in ("call", "import", "marcher", "library") and (read == "library") == (kind == "library"), name
        assert default == {"on": "1", "off": "0"}.get(kind, default), name
    assert sorted(n for n, row in switches.TABLE.items() if row[2] == "import") == ["HAVATAR_DEBUG_SYNC", "HAVATAR_NAN_TRACE"]
    assert sorted(n for n, row in switches.TABLE.items() if row[2] == "marcher") == ["HAVATAR_FINE_CACHE", "HAVATAR_MLP", "HAV_FINE", "HAV_MARCH"]
    assert {n: switches.default(n) for n in INT_DEFAULTS} == INT_DEFAULTS


@pytest.mark.parametrize("name", ON)
def test_on_switch(monkeypatch, name):
    for value, want in zip(VALUES, ON_EXPECT):
        _set(monkeypatch, name, value)
        assert switches.on(name) is want, (name, value)


@pytest.mark.parametrize("name", OFF)
def test_off_switch(monkeypatch, name):
    for value, want in zip(VALUES, OFF_EXPECT):
        _set(monkeypatch, name, value)
        assert switches.off(name) is want, (name, value)


def test_public_predicates(monkeypatch):
    from havatar_amd.harness import train
    from havatar_amd.model import styleUnet
    from havatar_amd.native import conv, lpips_ops, metrics_ops, train_ops
    on = (("HAVATAR_LPIPS", lpips_ops.enabled), ("HAVATAR_METRICS", metrics_ops.enabled), ("HAVATAR_S2_LOSS", train_ops.s2_loss_enabled),
          ("HAVATAR_FUSED_CONV", styleUnet._fused_conv_enabled), ("HAVATAR_FUSED_HAAR", styleUnet._fused_haar_enabled),
          ("HAVATAR_CONV_AUTOSCALE", conv._autoscale_default), ("HAVATAR_TRAIN_GRAPH", lambda: train.graph_training_enabled("cuda")),
          ("HAVATAR_HIP_TRAIN", lambda: train.graph_training_enabled("cuda")))
    off = (("HAVATAR_DETERMINISTIC", train_ops.deterministic), ("HAVATAR_DETERMINISTIC", train.deterministic_requested),
           ("HAVATAR_COMPOSITE_LONG", train_ops.composite_long_enabled), ("HAVATAR_HAAR_TRAIN", train_ops.haar_enabled))
    for n in ("HAVATAR_TRAIN_GRAPH", "HAVATAR_HIP_TRAIN"):
        monkeypatch.delenv(n, raising=False)
    for rows, expect in ((on, ON_EXPECT), (off, OFF_EXPECT)):
        for name, fn in rows:
            for value, want in zip(VALUES, expect):
                _set(monkeypatch, name, value)
                assert fn() is want, (name, value)
            monkeypatch.delenv(name, raising=False)
    assert train.graph_training_enabled("cpu") is False and train.graph_training_enabled("cuda", percep_loss_fn=object()) is False
    assert lpips_ops.DEFAULT == "1" and metrics_ops.DEFAULT == "1"


@pytest.mark.parametrize("name,value,want", CHOICE)
def test_choice_switch(monkeypatch, name, value, want):
    _set(monkeypatch, name, value)
    assert switches.choice(name) == want


def test_marcher_reads_its_four_when_it_is_built(monkeypatch):
    from havatar_amd import render
    assert render.DEFAULT_MLP == "mx" and render.MLP_MODES == {"mx": 3, "split": 0, "bf16": 0, "half": 2, "fp16": 2, "f32": 1}
    for n in ("HAVATAR_MLP", "HAVATAR_FINE_CACHE", "HAV_MARCH", "HAV_FINE"):
        monkeypatch.delenv(n, raising=False)
    box = ((1, 1, 1), (0, 0, 0), (1, 1, 1), (0, 0, 0))
    rm = render.RayMarcher(*box)
    assert (rm.mlp_mode, rm.fine_cache, rm.flags) == (3, True, 0)
    for env, want in (({"HAVATAR_MLP": "split"}, (0, True, 0)), ({"HAVATAR_MLP": "half"}, (2, True, 0)), ({"HAVATAR_MLP": "f32"}, (1, True, 0)),
                      ({"HAVATAR_MLP": "junk"}, (3, True, 0)), ({"HAVATAR_FINE_CACHE": "0"}, (3, False, 0)), ({"HAVATAR_FINE_CACHE": ""}, (3, True, 0)),
                      ({"HAV_MARCH": "pair"}, (3, True, 1)), ({"HAV_MARCH": "p"}, (3, True, 1)), ({"HAV_MARCH": "xp"}, (3, True, 0)),
                      ({"HAV_FINE": "cache"}, (3, True, 2)), ({"HAV_FINE": "recompute"}, (3, True, 4)), ({"HAV_FINE": "1"}, (3, True, 0)),
                      ({"HAV_MARCH": "pair", "HAV_FINE": "recompute"}, (3, True, 5))):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            new = render.RayMarcher(*box)
            assert (new.mlp_mode, new.fine_cache, new.flags) == want, env
            assert (rm.mlp_mode, rm.fine_cache, rm.flags) == (3, True, 0)          # a marcher built before does not follow


def test_int_switch(monkeypatch):
    for name, default in INT_DEFAULTS.items():
        monkeypatch.delenv(name, raising=False)
        if default is not None:
            assert switches.integer(name) == default
        monkeypatch.setenv(name, "5")
        assert switches.integer(name) == 5 and switches.integer(name, 8) == 5
        for junk in ("x", ""):
            monkeypatch.setenv(name, junk)
            with pytest.raises(ValueError):
                switches.integer(name)
    monkeypatch.delenv("HAVATAR_WORKERS")
    assert switches.integer("HAVATAR_WORKERS", 8) == 8 and switches.integer("HAVATAR_WORKERS", 4) == 4          # the harnesses' two defaults


def test_path_switch(monkeypatch):
    monkeypatch.delenv("HAVATAR_LIB", raising=False)
    assert switches.path("HAVATAR_LIB", "/default.so") == "/default.so"
    monkeypatch.setenv("HAVATAR_LIB", "/other.so")
    assert switches.path("HAVATAR_LIB", "/default.so") == "/other.so"


def test_unregistered_names_and_the_wrong_kind_raise(monkeypatch):
    monkeypatch.setenv("HAVATAR_NO_SUCH_SWITCH", "1")
    for fn in (switches.on, switches.off, switches.choice, switches.integer, switches.default):
        with pytest.raises(KeyError):
            fn("HAVATAR_NO_SUCH_SWITCH")
    with pytest.raises(KeyError):
        switches.path("HAVATAR_NO_SUCH_SWITCH", "x")
    for fn, name in ((switches.on, "HAVATAR_HAAR_TRAIN"), (switches.off, "HAVATAR_LPIPS"), (switches.on, "HAVATAR_MLP"), (switches.choice, "HAVATAR_LPIPS"),
                     (switches.integer, "HAVATAR_MLP"), (switches.choice, "HAVATAR_WORKERS"), (switches.choice, "HAVATAR_LIB"),
                     (switches.choice, "HAVATAR_UFD"), (switches.on, "HAV_ABLATE")):
        with pytest.raises(KeyError):
            fn(name)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. read at the call, but for the three module attributes
# ------------------------------------------------------------------------------------------------------------------------------------
def test_switches_are_read_at_the_call(monkeypatch):
    from havatar_amd import render
    from havatar_amd.native import conv, lpips_ops, train_ops
    sync, mode, trace = render._DEBUG_SYNC, conv._NAN_MODE, conv._NAN_TRACE
    for n in ("HAVATAR_LPIPS", "HAVATAR_HAAR_TRAIN", "HAVATAR_FUSED_TORGB"):
        monkeypatch.delenv(n, raising=False)
    assert (lpips_ops.enabled(), train_ops.haar_enabled(), switches.on("HAVATAR_FUSED_TORGB")) == (True, False, True)
    monkeypatch.setenv("HAVATAR_LPIPS", "0")
    monkeypatch.setenv("HAVATAR_HAAR_TRAIN", "1")
    monkeypatch.setenv("HAVATAR_FUSED_TORGB", "0")
    assert (lpips_ops.enabled(), train_ops.haar_enabled(), switches.on("HAVATAR_FUSED_TORGB")) == (False, True, False)
    for n in ("HAVATAR_LPIPS", "HAVATAR_HAAR_TRAIN", "HAVATAR_FUSED_TORGB"):
        monkeypatch.delenv(n)
    assert (lpips_ops.enabled(), train_ops.haar_enabled(), switches.on("HAVATAR_FUSED_TORGB")) == (True, False, True)
    monkeypatch.setenv("HAVATAR_DEBUG_SYNC", "0" if sync else "1")
    monkeypatch.setenv("HAVATAR_NAN_TRACE", "0" if mode else "2")
    assert render._DEBUG_SYNC is sync and conv._NAN_MODE == mode and conv._NAN_TRACE is trace
    assert switches.off("HAVATAR_DEBUG_SYNC") is not sync          # (the variable itself did change)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. one reading place;  4. table = code = README
# ------------------------------------------------------------------------------------------------------------------------------------
def _is_switch(node):
    return isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value.startswith(("HAVATAR_", "HAV_"))


def _is_environ(node):
    return (isinstance(node, ast.Attribute) and node.attr == "environ") or (isinstance(node, ast.Name) and node.id == "environ")


def _scan(src):
    """(direct reads of a switch from the environment, [(accessor, first argument node)]) of one module's source"""
    direct, calls = [], []
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Subscript) and _is_environ(node.value) and _is_switch(node.slice):
            direct.append((node.lineno, node.slice.value))
        elif isinstance(node, ast.Compare) and any(_is_environ(c) for c in node.comparators) and _is_switch(node.left):
            direct.append((node.lineno, node.left.value))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.args:
            f = node.func
            if ((f.attr in ("get", "setdefault", "pop") and _is_environ(f.value)) or f.attr == "getenv") and _is_switch(node.args[0]):
                direct.append((node.lineno, node.args[0].value))
            elif f.attr in ACCESSORS + ("default",) and isinstance(f.value, ast.Name) and f.value.id == "switches":
                calls.append((f.attr, node.args[0]))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getenv" and node.args and _is_switch(node.args[0]):
            direct.append((node.lineno, node.args[0].value))
    return direct, calls


def test_the_scan_sees_every_form():
    src = ('import os\nfrom os import environ, getenv\nimport os as _os\n'
           'a = os.environ["HAVATAR_A"]\nb = os.environ.get("HAVATAR_B", "1")\nc = _os.environ.setdefault("HAV_C", "0")\nd = "HAVATAR_D" in os.environ\n'
           'e = os.getenv("HAVATAR_E")\nf = environ.get("HAV_F")\ng = getenv("HAVATAR_G")\nh = "HAVATAR_H" not in environ\ni = os.environ.pop("HAVATAR_I", None)\n'
           'ok = os.environ.get("WORLD_SIZE", "1")\nalso_ok = os.environ.get("HIPCC")\nx = switches.on("HAVATAR_X")\ny = switches.integer(name)\n')
    direct, calls = _scan(src)
    assert sorted(n for _, n in direct) == ["HAVATAR_A", "HAVATAR_B", "HAVATAR_D", "HAVATAR_E", "HAVATAR_G", "HAVATAR_H", "HAVATAR_I", "HAV_C", "HAV_F"]
    assert [(a, type(n).__name__) for a, n in calls] == [("on", "Constant"), ("integer", "Name")]


def _package_scan():
    direct, calls = [], []
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        if os.path.relpath(path, PKG) == "switches.py":
            continue
        d, c = _scan(open(path).read())
        direct += [(os.path.relpath(path, ROOT),) + x for x in d]
        calls += [(os.path.relpath(path, ROOT),) + x for x in c]
    return direct, calls


def test_no_other_module_reads_a_switch_from_the_environment():
    direct, calls = _package_scan()
    assert direct == []
    assert len(calls) >= 56
    for path, accessor, arg in calls:
        assert isinstance(arg, ast.Constant) and isinstance(arg.value, str), (path, arg.lineno, "a switch is named by a string literal")
        assert arg.value in switches.TABLE, (path, arg.lineno, arg.value)
        if accessor != "default":
            assert switches.TABLE[arg.value][0] == {"integer": "int"}.get(accessor, accessor), (path, arg.lineno, arg.value)


def test_table_is_what_the_package_asks_for_and_what_the_library_reads():
    _, calls = _package_scan()
    asked = {arg.value for _, accessor, arg in calls if accessor != "default"}
    assert asked == {n for n, row in switches.TABLE.items() if row[0] != "library"}
    read = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")):
        read |= set(re.findall(r'getenv\("([^"]+)"\)', open(path).read()))
    assert read | {"HAV_ABLATE", "HAV_STAGGER"} == set(LIBRARY)


def test_table_is_readmes_table():
    text = open(os.path.join(ROOT, "README.md")).read()
    section = text.split("\n## Switches", 1)[1].split("\n## ", 1)[0]
    rows = [ln for ln in section.splitlines() if ln.startswith("|")][2:]
    assert len(rows) >= 40
    named = set()
    for ln in rows:
        named |= set(re.findall(r"\b(?:HAVATAR|HAV)_[A-Z0-9_]+", ln.split("|")[1]))
    assert named == set(switches.TABLE)
