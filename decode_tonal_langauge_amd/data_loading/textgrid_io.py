"""A small reader and writer of Praat TextGrid annotation files (the ``textgrid`` package is not a dependency).

Only what ``data_loading/text_align.py`` touches is offered: ``read_textgrid_file(path)`` returns a ``TextGrid`` with ``.tiers``;
each tier has ``.name`` and ``.intervals``; each interval has ``.minTime``, ``.maxTime`` and ``.mark``.

Both text formats are read - the long one (``item [1]: ... intervals [3]: xmin = ...``) and the short one (values only) - in
UTF-8 or, with a byte-order mark, UTF-16.  Both are a fixed sequence of values (numbers, quoted strings, ``<exists>``) between
labels that carry no information, so the file is cut into its values and the sequence is read off; a doubled quote inside a
mark is one quote.  Point tiers (``TextTier``) are parsed and skipped: ``.tiers`` holds interval tiers only.  A malformed
file raises ``ValueError`` naming the file and the line."""
from __future__ import annotations

import codecs
import re
from typing import List, NamedTuple, Sequence, Tuple, Union


class Interval(NamedTuple):
    minTime: float
    maxTime: float
    mark: str


class IntervalTier:
    def __init__(self, name: str, intervals: Sequence = (), minTime: float = None, maxTime: float = None) -> None:
        self.name = name
        self.intervals: List[Interval] = [Interval(float(a), float(b), str(m)) for a, b, m in intervals]
        self.minTime = float(minTime) if minTime is not None else (self.intervals[0].minTime if self.intervals else 0.0)
        self.maxTime = float(maxTime) if maxTime is not None else (self.intervals[-1].maxTime if self.intervals else 0.0)

    def __repr__(self) -> str:
        return f"IntervalTier({self.name!r}, {len(self.intervals)} intervals)"


class PointTier:
    """A ``TextTier``: ``points`` are ``(time, mark)``.  Written by ``write_textgrid``; skipped by the reader."""

    def __init__(self, name: str, points: Sequence = (), minTime: float = 0.0, maxTime: float = None) -> None:
        self.name = name
        self.points: List[Tuple[float, str]] = [(float(t), str(m)) for t, m in points]
        self.minTime = float(minTime)
        self.maxTime = float(maxTime) if maxTime is not None else (self.points[-1][0] if self.points else 0.0)


class TextGrid:
    def __init__(self, tiers: Sequence[IntervalTier] = (), minTime: float = 0.0, maxTime: float = 0.0) -> None:
        self.tiers: List[IntervalTier] = list(tiers)
        self.minTime, self.maxTime = float(minTime), float(maxTime)


# a value: a quoted string ("" inside is one quote; may span lines), a flag, or a number that starts a token.  Everything
# else - labels, "=", ":", the bracketed counters of the long format, "!" comments - is skipped.
_TOKEN = re.compile(r'"((?:[^"]|"")*)"|(<[A-Za-z]+>)|\[[^\]\n]*\]|![^\n]*|([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)'
                    r'|[A-Za-z_][\w?]*|(")|\s+|[^\s"]')


def _decode(raw: bytes, path: str) -> str:
    for bom, enc in ((codecs.BOM_UTF8, "utf-8"), (codecs.BOM_UTF16_LE, "utf-16-le"), (codecs.BOM_UTF16_BE, "utf-16-be")):
        if raw.startswith(bom):
            raw = raw[len(bom):]
            break
    else:
        enc = "utf-8"
    try:
        return raw.decode(enc)
    except UnicodeDecodeError as e:
        raise ValueError(f"{path}: not a {enc} text file ({e})") from None


class _Values:
    def __init__(self, text: str, path: str) -> None:
        self.path = path
        self.items = []                                   # (kind, value, line)
        line = 1
        for m in _TOKEN.finditer(text):
            if m.group(1) is not None:
                self.items.append(("string", m.group(1).replace('""', '"'), line))
            elif m.group(2) is not None:
                self.items.append(("flag", m.group(2), line))
            elif m.group(3) is not None:
                self.items.append(("number", m.group(3), line))
            elif m.group(4) is not None:
                raise ValueError(f"{path}: line {line}: a quoted string is not closed")
            line += m.group(0).count("\n")
        self.pos = 0
        self.last_line = line

    def take(self, kind: str, what: str):
        if self.pos >= len(self.items):
            raise ValueError(f"{self.path}: line {self.last_line}: the file ends where {what} is expected")
        k, v, line = self.items[self.pos]
        if k != kind:
            raise ValueError(f"{self.path}: line {line}: expected {what} (a {kind}), found the {k} {v!r}")
        self.pos += 1
        return v, line

    def number(self, what: str) -> float:
        return float(self.take("number", what)[0])

    def count(self, what: str) -> int:
        v, line = self.take("number", what)
        try:
            n = int(v)
        except ValueError:
            n = -1
        if n < 0:
            raise ValueError(f"{self.path}: line {line}: {what} must be a non-negative integer, found {v!r}")
        return n

    def string(self, what: str) -> str:
        return self.take("string", what)[0]


def parse_textgrid(raw: bytes, path: str = "<bytes>") -> TextGrid:
    v = _Values(_decode(raw, path), path)
    file_type, line = v.take("string", 'the file type "ooTextFile"')
    if file_type != "ooTextFile":
        raise ValueError(f'{path}: line {line}: file type {file_type!r} is not "ooTextFile"')
    cls, line = v.take("string", 'the object class "TextGrid"')
    if cls != "TextGrid":
        raise ValueError(f'{path}: line {line}: object class {cls!r} is not "TextGrid"')
    xmin, xmax = v.number("xmin of the file"), v.number("xmax of the file")
    grid = TextGrid([], xmin, xmax)
    flag, line = v.take("flag", "the <exists> flag of the tiers")
    if flag != "<exists>":
        return grid
    for t in range(v.count("the number of tiers")):
        kind, line = v.take("string", f"the class of tier {t + 1}")
        name = v.string(f"the name of tier {t + 1}")
        tmin, tmax = v.number(f"xmin of tier {name!r}"), v.number(f"xmax of tier {name!r}")
        if kind == "IntervalTier":
            rows = []
            for i in range(v.count(f"the number of intervals of tier {name!r}")):
                what = f"interval {i + 1} of tier {name!r}"
                rows.append((v.number(f"xmin of {what}"), v.number(f"xmax of {what}"), v.string(f"the text of {what}")))
            grid.tiers.append(IntervalTier(name, rows, tmin, tmax))
        elif kind == "TextTier":
            for i in range(v.count(f"the number of points of tier {name!r}")):
                what = f"point {i + 1} of tier {name!r}"
                v.number(f"the time of {what}")
                v.string(f"the mark of {what}")
        else:
            raise ValueError(f"{path}: line {line}: unknown tier class {kind!r}")
    return grid


def read_textgrid_file(path: str) -> TextGrid:
    with open(path, "rb") as f:
        return parse_textgrid(f.read(), str(path))


def _q(s: str) -> str:
    return '"' + str(s).replace('"', '""') + '"'


def _tiers(tiers) -> List[Union[IntervalTier, PointTier]]:
    return [t if isinstance(t, (IntervalTier, PointTier)) else IntervalTier(t[0], t[1]) for t in tiers]


def write_textgrid(path: str, tiers, short: bool = False, encoding: str = "utf-8") -> str:
    """Write interval tiers - ``IntervalTier`` objects or ``(name, [(xmin, xmax, mark), ...])`` pairs - and ``PointTier``
    objects as a TextGrid in the long format, or the short one.  ``encoding``: ``"utf-8"`` (no byte-order mark) or
    ``"utf-16"`` (with one).  Times are written with ``repr``: reading the file back gives the same floats."""
    tiers = _tiers(tiers)
    xmin = min([t.minTime for t in tiers], default=0.0)
    xmax = max([t.maxTime for t in tiers], default=0.0)
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', ""]
    if short:
        out += [repr(xmin), repr(xmax), "<exists>", str(len(tiers))]
        for t in tiers:
            point = isinstance(t, PointTier)
            rows = t.points if point else t.intervals
            out += [_q("TextTier" if point else "IntervalTier"), _q(t.name), repr(t.minTime), repr(t.maxTime), str(len(rows))]
            for row in rows:
                out += [repr(x) for x in row[:-1]] + [_q(row[-1])]
    else:
        out += [f"xmin = {xmin!r} ", f"xmax = {xmax!r} ", "tiers? <exists> ", f"size = {len(tiers)} ", "item []: "]
        for k, t in enumerate(tiers):
            point = isinstance(t, PointTier)
            rows = t.points if point else t.intervals
            word = "points" if point else "intervals"
            out += [f"    item [{k + 1}]:", f'        class = {_q("TextTier" if point else "IntervalTier")} ',
                    f"        name = {_q(t.name)} ", f"        xmin = {t.minTime!r} ", f"        xmax = {t.maxTime!r} ",
                    f"        {word}: size = {len(rows)} "]
            for i, row in enumerate(rows):
                out.append(f"        {word} [{i + 1}]:")
                if point:
                    out += [f"            number = {row[0]!r} ", f"            mark = {_q(row[1])} "]
                else:
                    out += [f"            xmin = {row[0]!r} ", f"            xmax = {row[1]!r} ",
                            f"            text = {_q(row[2])} "]
    if encoding.lower().replace("_", "-") not in ("utf-8", "utf-16"):
        raise ValueError(f"write_textgrid: encoding must be 'utf-8' or 'utf-16', got {encoding!r}")
    with open(path, "wb") as f:
        f.write(("\n".join(out) + "\n").encode(encoding))          # Python's "utf-16" writes the byte-order mark
    return str(path)
