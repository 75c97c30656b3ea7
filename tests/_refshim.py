"""The read-only reference implementation as a numerical oracle for the parity tests, replayed
from recorded results.

The parity tests call the reference's Python code (``mfm.CrossSection``, ``mfm.utils``,
``mfm.MFM``, ``Barra_factor_cal``'s ``factor_calculator`` / ``post_processing`` and the legacy
``factor.py``) on inputs they generate themselves from fixed seeds.  What those calls return is
recorded once, per test, under ``tests/golden/reference/`` (one ``.npz`` of plain arrays and a
JSON manifest per test: no pickles, no code), and the suite replays the records: ``ref.x.y(...)``
returns what the reference returned for the same call of the same test, in call order.  The
suite therefore needs neither the reference checkout nor ``statsmodels``.

Recording (only when a test's inputs or its reference calls change)::

    MFA_REFERENCE=/path/to/reference MFA_RECORD_REFERENCE=1 python -m pytest tests -m reference

runs the reference's ``.py`` sources themselves (nothing prebuilt) and rewrites the records of the
tests that ran.  ``statsmodels`` is not a dependency of this repository, so a minimal,
formula-faithful stub is installed for the duration of the import: ``DescrStatsW(x,
weights).mean`` (weighted column mean), and ``statsmodels.api`` ``add_constant`` / ``WLS`` /
``OLS`` backed by a weighted least-squares solve that reports ``params``, ``resid`` (unweighted,
``y - X b``) and ``scale`` (``sum w e^2 / (n - k)``) exactly as statsmodels defines them.  The
reference's top-level package is also named ``mfm``; it is loaded under its own name and
``sys.modules`` is restored afterwards so it never shadows this repo's ``mfm`` package.
"""
from __future__ import annotations

import contextlib
import importlib
import importlib.util
import json
import os
import re
import sys
import types
from types import SimpleNamespace

import numpy as np
import pandas as pd

REF = os.environ.get("MFA_REFERENCE", "")
RECORD = bool(os.environ.get("MFA_RECORD_REFERENCE"))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")


class _DescrStatsW:
    def __init__(self, data, weights=None, ddof=0):
        self.data = np.asarray(data, dtype=float)
        self.weights = np.ones(len(self.data)) if weights is None else np.asarray(weights, dtype=float)

    @property
    def mean(self):
        w = self.weights
        return (self.data * w.reshape((-1,) + (1,) * (self.data.ndim - 1))).sum(0) / w.sum()


class _Fit:
    def __init__(self, y, X, w):
        yv = np.asarray(y, dtype=float)
        Xv = np.asarray(X, dtype=float)
        sw = np.sqrt(np.asarray(w, dtype=float))
        b, *_ = np.linalg.lstsq(Xv * sw[:, None], yv * sw, rcond=None)
        e = yv - Xv @ b
        n, k = Xv.shape
        names = list(X.columns) if isinstance(X, pd.DataFrame) else list(range(k))
        idx = y.index if isinstance(y, pd.Series) else None
        self.params = pd.Series(b, index=names)
        self.resid = pd.Series(e, index=idx) if idx is not None else e
        self.scale = float((np.asarray(w) * e * e).sum() / (n - k))


class _WLS:
    def __init__(self, y, X, weights=1.0):
        self.y, self.X = y, X
        self.w = np.broadcast_to(np.asarray(weights, dtype=float), (len(y),))

    def fit(self):
        return _Fit(self.y, self.X, self.w)


class _OLS(_WLS):
    def __init__(self, y, X):
        super().__init__(y, X, 1.0)


def _add_constant(x):
    if isinstance(x, pd.Series):
        x = x.to_frame()
    if isinstance(x, pd.DataFrame):
        out = x.copy()
        out.insert(0, "const", 1.0)
        return out
    x = np.asarray(x, dtype=float)
    return np.column_stack([np.ones(len(x)), x])


def _install_statsmodels_stub():
    if "statsmodels" in sys.modules and not getattr(sys.modules["statsmodels"], "_mfa_stub", False):
        return
    sm = types.ModuleType("statsmodels"); sm._mfa_stub = True; sm.__path__ = []
    stats = types.ModuleType("statsmodels.stats"); stats.__path__ = []
    ws = types.ModuleType("statsmodels.stats.weightstats")
    ws.DescrStatsW = _DescrStatsW
    api = types.ModuleType("statsmodels.api")
    api.add_constant, api.WLS, api.OLS = _add_constant, _WLS, _OLS
    sm.stats, sm.api, stats.weightstats = stats, api, ws
    sys.modules.update({"statsmodels": sm, "statsmodels.stats": stats,
                        "statsmodels.stats.weightstats": ws, "statsmodels.api": api})


def _load_live():
    """Import the reference's sources (recording only)."""
    mdir = os.path.join(REF, "Barra-master", "mfm")
    if not REF or not os.path.isdir(mdir):
        raise RuntimeError("MFA_RECORD_REFERENCE needs MFA_REFERENCE=<reference checkout>")
    _install_statsmodels_stub()
    import matplotlib
    matplotlib.use("Agg")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "mfm" or k.startswith("mfm.")}
    old_dwb = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        pkg = types.ModuleType("mfm")
        pkg.__path__ = [mdir]
        sys.modules["mfm"] = pkg
        cs = importlib.import_module("mfm.CrossSection")
        ut = importlib.import_module("mfm.utils")
        mf = importlib.import_module("mfm.MFM")
        fc_dir = os.path.join(REF, "Barra_factor_cal")
        sys.path.insert(0, fc_dir)
        try:
            fc = importlib.import_module("factor_calculator")
            pp = importlib.import_module("post_processing")
        finally:
            sys.path.remove(fc_dir)
            for k in ("factor_calculator", "post_processing"):
                sys.modules.pop(k, None)
        # legacy CSV-era twin at the reference's root (/factor.py)
        legacy = None
        if os.path.isfile(os.path.join(REF, "factor.py")):
            spec = importlib.util.spec_from_file_location("_mfa_ref_legacy_factor",
                                                          os.path.join(REF, "factor.py"))
            legacy = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(legacy)
    finally:
        for k in [k for k in sys.modules if k == "mfm" or k.startswith("mfm.")]:
            sys.modules.pop(k)
        sys.modules.update(saved)
        sys.dont_write_bytecode = old_dwb
    return SimpleNamespace(CrossSection=cs, utils=ut, MFM=mf, factor_calculator=fc,
                           post_processing=pp, legacy_factor=legacy)


# ---- records: a value tree of plain data <-> (JSON manifest, list of arrays) -------------------

def _arr(a, arrays):
    a = np.asarray(a)
    if a.dtype == object:   # strings (stock codes, column names): fixed-width unicode, no pickle
        if not all(isinstance(x, str) for x in a.reshape(-1)):
            raise TypeError(f"cannot record an object array of {set(map(type, a.reshape(-1)))}")
        a = a.astype(str)
    arrays.append(a)
    return len(arrays) - 1


def _enc_index(ix, arrays):
    if isinstance(ix, pd.RangeIndex):
        return {"range": [ix.start, ix.stop, ix.step], "name": ix.name}
    if isinstance(ix, pd.MultiIndex):
        raise TypeError("cannot record a MultiIndex")
    return {"a": _arr(ix.to_numpy(), arrays), "obj": ix.dtype == object, "name": ix.name}


def _dec_index(m, arrays):
    if "range" in m:
        return pd.RangeIndex(*m["range"], name=m["name"])
    a = arrays[m["a"]]
    return pd.Index(a.astype(object) if m["obj"] else a, name=m["name"])


def _encode(v, arrays, handle):
    if v is None or isinstance(v, (bool, int, str)):
        return {"py": v}
    if isinstance(v, float):
        return {"float": v}   # JSON floats round-trip exactly
    if isinstance(v, np.generic):
        return {"scalar": _arr(v, arrays)}
    if isinstance(v, np.matrix):
        return {"matrix": _arr(np.asarray(v), arrays)}
    if isinstance(v, np.ndarray):
        return {"ndarray": _arr(v, arrays), "obj": v.dtype == object}
    if isinstance(v, pd.Series):
        return {"series": _arr(v.to_numpy(), arrays), "obj": v.dtype == object,
                "index": _enc_index(v.index, arrays), "name": v.name}
    if isinstance(v, pd.DataFrame):
        if v.shape[1] and v.dtypes.nunique() == 1 and v.dtypes.iloc[0] != object:
            return {"frame2d": _arr(v.to_numpy(), arrays), "columns": _enc_index(v.columns, arrays),
                    "index": _enc_index(v.index, arrays)}
        cols = [{"a": _arr(v.iloc[:, j].to_numpy(), arrays), "obj": v.dtypes.iloc[j] == object}
                for j in range(v.shape[1])]
        return {"frame": cols, "columns": _enc_index(v.columns, arrays),
                "index": _enc_index(v.index, arrays)}
    if isinstance(v, (tuple, list)):
        return {"seq": [_encode(x, arrays, handle) for x in v], "tuple": isinstance(v, tuple)}
    if isinstance(v, dict) and all(isinstance(k, str) for k in v):
        return {"dict": {k: _encode(x, arrays, handle) for k, x in v.items()}}
    return {"handle": handle(v)}


def _decode(m, arrays, handle):
    def col(a, obj):
        return a.astype(object) if obj else a
    if "py" in m:
        return m["py"]
    if "float" in m:
        return float(m["float"])
    if "scalar" in m:
        return arrays[m["scalar"]][()]
    if "matrix" in m:
        return np.matrix(arrays[m["matrix"]])
    if "ndarray" in m:
        return col(arrays[m["ndarray"]], m["obj"])
    if "series" in m:
        return pd.Series(col(arrays[m["series"]], m["obj"]), index=_dec_index(m["index"], arrays),
                         name=m["name"])
    if "frame2d" in m:
        return pd.DataFrame(arrays[m["frame2d"]], index=_dec_index(m["index"], arrays),
                            columns=_dec_index(m["columns"], arrays))
    if "frame" in m:
        index = _dec_index(m["index"], arrays)
        df = pd.DataFrame({j: pd.Series(col(arrays[c["a"]], c["obj"]), index=index)
                           for j, c in enumerate(m["frame"])}, index=index)
        df.columns = _dec_index(m["columns"], arrays)
        return df
    if "seq" in m:
        out = [_decode(x, arrays, handle) for x in m["seq"]]
        return tuple(out) if m["tuple"] else out
    if "dict" in m:
        return {k: _decode(x, arrays, handle) for k, x in m["dict"].items()}
    return handle(m["handle"])


# ---- the tape: per test, the reference calls / attribute reads in order -------------------------

_CURRENT = [None]     # id of the running test (tests/conftest.py) or an explicit scope()
_TAPES = {}           # id -> {"events": [...], "arrays": [...], "pos": int, "objs": [...]}


def _file(test_id):
    return os.path.join(GOLDEN, re.sub(r"[^A-Za-z0-9_.-]+", "_", test_id).strip("_") + ".npz")


def _tape():
    tid = _CURRENT[0]
    if tid is None:
        raise RuntimeError("reference call outside a test (see tests/_refshim.scope)")
    if tid not in _TAPES:
        t = {"events": [], "arrays": [], "pos": 0, "objs": []}
        if not RECORD:
            if not os.path.isfile(_file(tid)):
                raise FileNotFoundError(f"no recorded reference results for {tid}: {_file(tid)} "
                                        "(record them, see tests/_refshim.py)")
            with np.load(_file(tid), allow_pickle=False) as z:
                t["events"] = json.loads(str(z["manifest"][()]))
                t["arrays"] = [z[f"a{i}"] for i in range(len(z.files) - 1)]
        _TAPES[tid] = t
    return _TAPES[tid]


def test_id(item):
    """Record name of a pytest item: ``<module>::<test>[<case>]``."""
    return f"{item.module.__name__.rsplit('.', 1)[-1]}::{item.name}"


def set_current_test(test_id):
    _CURRENT[0] = test_id


def finish_test(test_id):
    """Recording: write the test's tape."""
    t = _TAPES.pop(test_id, None)
    if t is not None and RECORD and t["events"]:
        os.makedirs(GOLDEN, exist_ok=True)
        arrays = {f"a{i}": a for i, a in enumerate(t["arrays"])}
        np.savez_compressed(_file(test_id), manifest=np.array(json.dumps(t["events"])), **arrays)


@contextlib.contextmanager
def scope(name):
    """Reference calls made inside belong to the record ``name`` instead of the running test's
    (a module-scoped fixture shared by several tests)."""
    old = _CURRENT[0]
    _CURRENT[0] = name
    try:
        yield
    finally:
        finish_test(name)
        _CURRENT[0] = old


_OPAQUE = [False]


@contextlib.contextmanager
def intermediate():
    """Results of the reference calls made inside are only handed on to later reference calls:
    they are recorded as opaque handles, not as data (a large intermediate frame)."""
    old = _OPAQUE[0]
    _OPAQUE[0] = True
    try:
        yield
    finally:
        _OPAQUE[0] = old


def _is_data(v):
    return v is None or isinstance(v, (bool, int, float, str, np.generic, np.ndarray, pd.Series,
                                       pd.DataFrame, tuple, list, dict))


class _Ref:
    """``ref`` or something reached from it: a module, a class, a function, an instance."""

    def __init__(self, path, live=None):
        object.__setattr__(self, "_path", path)
        object.__setattr__(self, "_live", live)

    def _wrap(self, t, v):
        def handle(obj):
            t["objs"].append(obj)
            return len(t["objs"]) - 1
        return {"handle": handle(v)} if _OPAQUE[0] else _encode(v, t["arrays"], handle)

    def _unwrap(self, t, m):
        return _decode(m, t["arrays"], lambda n: _Ref(f"#{n}", t["objs"][n] if RECORD else None))

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        path = f"{self._path}.{name}"
        if RECORD:
            v = getattr(self._live, name)
            if not _is_data(v):
                return _Ref(path, v)
            t = _tape()
            m = self._wrap(t, v)
            t["events"].append({"get": path, "value": m})
            return self._unwrap(t, m)
        t = _tape() if _CURRENT[0] is not None else None
        if t is not None and t["pos"] < len(t["events"]) and t["events"][t["pos"]].get("get") == path:
            t["pos"] += 1
            return self._unwrap(t, t["events"][t["pos"] - 1]["value"])
        return _Ref(path)

    def __setattr__(self, name, value):
        if RECORD:   # e.g. a stage's input replaced by the test; replay returns what followed
            setattr(self._live, name, value)

    def __call__(self, *args, **kwargs):
        t = _tape()
        if RECORD:
            args = [a._live if isinstance(a, _Ref) else a for a in args]
            m = self._wrap(t, self._live(*args, **kwargs))
            t["events"].append({"call": self._path, "value": m})
            return self._unwrap(t, m)
        if t["pos"] >= len(t["events"]) or t["events"][t["pos"]].get("call") != self._path:
            want = t["events"][t["pos"]] if t["pos"] < len(t["events"]) else None
            raise AssertionError(f"reference call {self._path} does not follow the record "
                                 f"(next recorded: {want and (want.get('call') or want.get('get'))})")
        t["pos"] += 1
        return self._unwrap(t, t["events"][t["pos"] - 1]["value"])


_CACHE = {}


def load_reference():
    if "ref" not in _CACHE:
        _CACHE["ref"] = _Ref("ref", _load_live() if RECORD else None)
    return _CACHE["ref"]


def reference_source(*parts):
    """Recording only: path of a file of the reference checkout."""
    return os.path.join(REF, *parts)
