"""Every HAVATAR_* / HAV_* environment switch, in one table, and the only functions of the Python layer that read one.

Kinds (the accessor of the same name; `integer` for "int"):
  on       on unless the value is exactly "0"
  off      on only if the value is exactly "1"
  choice   the raw string (the default when unset); the caller compares it
  int      int(value): a junk or empty value raises ValueError
  path     the raw string
  library  read by getenv inside csrc/, once per process, never by Python: no accessor

Read: "call" = at every call of the code that asks (tests flip these between calls); "import" = once, into a module attribute;
"marcher" = when a render.RayMarcher is built; "library" = see above.  Nothing is cached here.  A default of None means the caller
passes its own.  An unregistered name, or a name asked for through another kind's accessor, raises KeyError.

To add a switch: one row here, one accessor call where it acts, one row in README's "Switches" table (tests/test_switches.py holds the three
together).  Importing only `os` keeps this module usable from _lib.py and build.py.
"""
import os

TABLE = {
    # name: (kind, default, read)
    "HAVATAR_LIB": ("path", None, "call"),
    "HAVATAR_REQUIRE_TESTED_HIPCC": ("off", "0", "call"),
    "HAVATAR_GRAPH_SHAPE": ("off", "0", "call"),
    "HAVATAR_DEBUG_SYNC": ("off", "0", "import"),
    "HAVATAR_NAN_TRACE": ("choice", "", "import"),          # conv._NAN_MODE; harness/train.py asks again per logged step
    # render.RayMarcher
    "HAVATAR_MLP": ("choice", "mx", "marcher"),
    "HAVATAR_FINE_CACHE": ("on", "1", "marcher"),
    "HAV_MARCH": ("choice", "", "marcher"),
    "HAV_FINE": ("choice", "", "marcher"),
    # native/
    "HAVATAR_LPIPS": ("on", "1", "call"),
    "HAVATAR_METRICS": ("on", "1", "call"),
    "HAVATAR_CONV_AUTOSCALE": ("on", "1", "call"),
    "HAVATAR_S2_WGRAD": ("on", "1", "call"),
    "HAVATAR_CONV_BWD": ("on", "1", "call"),
    "HAVATAR_CONV_WGRAD": ("on", "1", "call"),
    "HAVATAR_FUSED_BLOCK": ("on", "1", "call"),
    "HAVATAR_S2_TRAIN_FWD": ("choice", "kernel", "call"),
    "HAVATAR_S2_DGRAD": ("on", "1", "call"),
    "HAVATAR_FUSED_UPBLOCK": ("on", "1", "call"),
    "HAVATAR_DETERMINISTIC": ("off", "0", "call"),
    "HAVATAR_COMPOSITE_LONG": ("off", "0", "call"),
    "HAVATAR_CONV3D_SMALL": ("on", "1", "call"),
    "HAVATAR_HAAR_TRAIN": ("off", "0", "call"),
    "HAVATAR_S2_LOSS": ("on", "1", "call"),
    # model/
    "HAVATAR_HIP_TRAIN": ("on", "1", "call"),
    "HAVATAR_FUSED_CONV": ("on", "1", "call"),
    "HAVATAR_EQUAL_LINEAR": ("on", "1", "call"),
    "HAVATAR_FUSED_UPCONV": ("on", "1", "call"),
    "HAVATAR_CONV_S2": ("on", "1", "call"),
    "HAVATAR_S2_INFER": ("on", "1", "call"),
    "HAVATAR_S2_TRAIN": ("on", "1", "call"),
    "HAVATAR_CONV_1X1": ("off", "0", "call"),
    "HAVATAR_FUSED_HAAR": ("on", "1", "call"),
    "HAVATAR_FUSED_TORGB": ("on", "1", "call"),
    "HAVATAR_STYLE_BATCH": ("on", "1", "call"),
    "HAVATAR_STYLE_MLP": ("on", "1", "call"),
    "HAVATAR_CONV3D": ("choice", "", "call"),
    "HAVATAR_DECODER": ("choice", "", "call"),
    "HAVATAR_TRAIN_CHUNK_RAYS": ("int", 32768, "call"),
    "HAVATAR_TRAIN_MLP": ("choice", "bf16", "call"),
    "HAVATAR_FIELD_MLP": ("on", "1", "call"),
    "HAVATAR_FIELD_ROWS": ("off", "0", "call"),
    "HAVATAR_RESAMPLE": ("choice", "hip", "call"),
    "HAVATAR_ENC_STREAMS": ("on", "1", "call"),
    "HAVATAR_HIP_GATHER": ("on", "1", "call"),
    # harness/
    "HAVATAR_TRAIN_GRAPH": ("on", "1", "call"),
    "HAVATAR_FUSED_ADAM": ("on", "1", "call"),
    "HAVATAR_DET_MIOPEN": ("on", "1", "call"),
    "HAVATAR_DET_ATEN": ("on", "1", "call"),
    "HAVATAR_GRAPH_CAPTURE_STREAM": ("choice", "", "call"),
    "HAVATAR_WORKERS": ("int", None, "call"),          # 8 in the training harnesses, 4 in reenact.py
    "HAVATAR_PRETRAIN_WC": ("int", 3000, "call"),
    "HAVATAR_DEVICE_RAYS": ("on", "1", "call"),
    "HAVATAR_FRAME_BATCH": ("int", 1, "call"),
    "HAVATAR_GRAPH": ("on", "1", "call"),
    "HAVATAR_PNG_THREADS": ("int", 12, "call"),
    # csrc/
    "HAVATAR_UFD": ("library", None, "library"),
    "HAVATAR_UFD_SEG": ("library", None, "library"),
    "HAVATAR_UFD_DOWN2": ("library", None, "library"),
    "HAVATAR_CONV_KERNEL": ("library", None, "library"),
    "HAVATAR_CONV_KSPLIT_CUS": ("library", None, "library"),
    "HAVATAR_FIELD_BWD": ("library", None, "library"),
    "HAVATAR_COMPOSITE_BWD": ("library", None, "library"),
    "HAV_ABLATE": ("library", None, "library"),          # lab builds only (csrc/hav_render_lab.h)
    "HAV_STAGGER": ("library", None, "library"),
}


def _get(name, kind, default=None):
    k, d, _ = TABLE[name]
    if k != kind:
        raise KeyError("%s is a switch of kind %r, not %r" % (name, k, kind))
    return os.environ.get(name, d if default is None else default)


def on(name):
    return _get(name, "on") != "0"


def off(name):
    return _get(name, "off") == "1"


def choice(name):
    return _get(name, "choice")


def integer(name, default=None):
    return int(_get(name, "int", default))


def path(name, default):
    return _get(name, "path", default)


def default(name):
    """the table's default, as the string (or int) an unset variable stands for"""
    return TABLE[name][1]
