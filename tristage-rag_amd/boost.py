"""Boost specs of the boosted stage-1 search: from a spec and the documents' metadata to the per-document
bias ``FlatIPIndex.search_biased`` adds to every score.  Pure host code (numpy only): every formula is evaluated in
float64 and the result is rounded to float32 once.

A spec is one of

* a float array with one entry per document, already scaled (a wrong length is a ``ValueError``);
* ``{"field": key, "weight": w, "missing": 0.0}``: the bias of a document is ``w * float(metadata[key])``;
* ``{"field": key, "decay": "exp" | "gauss" | "linear", "origin": o, "scale": s, "offset": 0.0, "decay_value": 0.5,
  "weight": w, "missing": 0.0}``: ``w * f(max(0, |float(metadata[key]) - o| - offset))`` with Elasticsearch's decay
  functions: ``f(0) = 1`` and ``f(s) = decay_value``,

      exp     f(x) = exp(x * ln(decay_value) / s)
      gauss   f(x) = exp(x^2 * ln(decay_value) / s^2)
      linear  f(x) = max(0, 1 - x * (1 - decay_value) / s)

* a callable ``metadata -> float``.

A document whose metadata lacks ``key`` (or holds None there) gets the bias ``missing`` as it is: it is a bias, not a
field value, so neither the weight nor the decay is applied to it.  ``weight`` defaults to 1.  Every bias must be finite
(``ValueError``)."""
import math
from typing import Any, Callable, Hashable, Sequence, Tuple

import numpy as np

DECAYS = ("exp", "gauss", "linear")
_FIELD_KEYS = {"field", "weight", "missing"}
_DECAY_KEYS = _FIELD_KEYS | {"decay", "origin", "scale", "offset", "decay_value"}


def check_spec(spec) -> None:
    """``ValueError`` / ``TypeError`` for a spec no bias can be made of; needs no documents."""
    if callable(spec):
        return
    if isinstance(spec, dict):
        if "field" not in spec:
            raise ValueError('a boost dict needs a "field"')
        allowed = _DECAY_KEYS if "decay" in spec else _FIELD_KEYS
        extra = sorted(set(spec) - allowed)
        if extra:
            raise ValueError(f"unknown boost keys {extra} (a {'decay' if 'decay' in spec else 'field'} boost takes "
                             f"{sorted(allowed)})")
        for key in ("weight", "missing", "origin", "scale", "offset", "decay_value"):
            if key in spec and not math.isfinite(float(spec[key])):
                raise ValueError(f"boost {key} must be finite, got {spec[key]!r}")
        if "decay" in spec:
            if spec["decay"] not in DECAYS:
                raise ValueError(f"boost decay must be one of {DECAYS}, got {spec['decay']!r}")
            if "origin" not in spec or "scale" not in spec:
                raise ValueError('a decay boost needs "origin" and "scale"')
            if not float(spec["scale"]) > 0.0:
                raise ValueError(f"boost scale must be positive, got {spec['scale']!r}")
            if float(spec.get("offset", 0.0)) < 0.0:
                raise ValueError(f"boost offset must not be negative, got {spec['offset']!r}")
            if not 0.0 < float(spec.get("decay_value", 0.5)) < 1.0:
                raise ValueError(f"boost decay_value must be in (0, 1), got {spec['decay_value']!r}")
        return
    arr = np.asarray(spec)
    if arr.ndim != 1 or arr.dtype.kind not in "fiu":
        raise TypeError(f"a boost is a 1-D numeric array, a dict or a callable, got {type(spec).__name__}")


def spec_key(spec) -> Tuple[Hashable, Any]:
    """``(key, keep)``: a hashable key of the spec for the retriever's cache and the object that has to stay alive while
    the key is in use (an array or a callable is told apart by identity)."""
    if isinstance(spec, dict):
        return ("dict",) + tuple(sorted((str(k), repr(v)) for k, v in spec.items())), None
    return ("id", id(spec)), spec


def decay(kind: str, x: float, scale: float, decay_value: float) -> float:
    """Elasticsearch's decay functions of the distance ``x >= 0`` (float64)."""
    if kind == "exp":
        return math.exp(x * math.log(decay_value) / scale)
    if kind == "gauss":
        return math.exp(x * x * math.log(decay_value) / (scale * scale))
    if kind == "linear":
        return max(0.0, 1.0 - x * (1.0 - decay_value) / scale)
    raise ValueError(f"boost decay must be one of {DECAYS}, got {kind!r}")


def _field_fn(spec: dict) -> Callable[[Any], float]:
    key = spec["field"]
    w = float(spec.get("weight", 1.0))
    missing = float(spec.get("missing", 0.0))
    kind = spec.get("decay")
    if kind is not None:
        origin, scale = float(spec["origin"]), float(spec["scale"])
        offset, dv = float(spec.get("offset", 0.0)), float(spec.get("decay_value", 0.5))

    def fn(meta) -> float:
        v = meta.get(key) if isinstance(meta, dict) else None
        if v is None:
            return missing
        x = float(v)
        if kind is None:
            return w * x
        return w * decay(kind, max(0.0, abs(x - origin) - offset), scale, dv)
    return fn


def bias_array(spec, metadata: Sequence[Any]) -> np.ndarray:
    """The float32 bias of ``spec`` over the documents whose metadata is ``metadata`` (one entry each)."""
    check_spec(spec)
    n = len(metadata)
    if callable(spec) or isinstance(spec, dict):
        fn = spec if callable(spec) else _field_fn(spec)
        b64 = np.fromiter((float(fn(m)) for m in metadata), dtype=np.float64, count=n)
    else:
        b64 = np.asarray(spec, dtype=np.float64)
        if b64.shape != (n,):
            raise ValueError(f"a boost array holds one entry per document, [{n}], got {tuple(b64.shape)}")
    with np.errstate(over="ignore"):
        b = np.ascontiguousarray(b64.astype(np.float32))
    if not np.isfinite(b).all():
        bad = int(np.flatnonzero(~np.isfinite(b))[0])
        raise ValueError(f"the boost of document {bad} is not a finite float32 ({b64[bad]!r})")
    return b
