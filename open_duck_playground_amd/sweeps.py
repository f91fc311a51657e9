"""What every sweep flag of `track` shares (`--grid`, `--push_grid`, `--plant` / `--plant_grid`, `--sensor` / `--sensor_grid`): the
`NAME=start:stop:count,...` and `KEY=V,...` syntaxes and the env layout of the cells.  Host code only: no GPU, no torch."""
from __future__ import annotations

import itertools
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np


def parse_axis_grid(flag: str, spec: str, names: Sequence[str], noun: str = "axis", value: Optional[Callable] = None,
                    check: Optional[Callable] = None, refused: Optional[Dict[str, str]] = None, required: Optional[str] = None) -> List[Tuple[str, List]]:
    """`NAME=a:b:n,NAME=c:d:m` -> the (name, values) axes in the order written: each axis takes n values from a to b (numpy.linspace, ends
    included).  ValueError, as `flag`'s, for a name that is not one of `names` (a `noun`: "axis" or "key"), a name given twice, a range
    that is not start:stop:count, a count below 1 and a spec without an axis (without the `required` one, for a flag that has one).  What
    a flag adds: `refused`, the reason by name for the names that are no grid axis; `check(name, part, lo, hi)`, which raises for a range
    the flag does not take; `value(flag, name, v)`, which gives each value as the flag holds it or raises."""
    axes = []
    for part in str(spec).split(","):
        part = part.strip()
        if not part:
            continue
        name, _, rng = part.partition("=")
        name = name.strip()
        if name not in names:
            raise ValueError(f"{flag}: unknown {noun} {name!r} (one of {', '.join(names)})")
        if refused and name in refused:
            raise ValueError(f"{flag}: {refused[name]}")
        if any(name == a for a, _ in axes):
            raise ValueError(f"{flag}: {noun} {name!r} given twice")
        bits = rng.split(":")
        try:
            lo, hi, n = float(bits[0]), float(bits[1]), int(bits[2])
            assert len(bits) == 3
        except (ValueError, IndexError, AssertionError):
            raise ValueError(f"{flag}: {part!r} is not {name}=start:stop:count")
        if n < 1:
            raise ValueError(f"{flag}: {part!r} needs a count >= 1")
        if check is not None:
            check(name, part, lo, hi)
        values = np.linspace(lo, hi, n).tolist()
        axes.append((name, values if value is None else [value(flag, name, v) for v in values]))
    if not axes or (required is not None and all(name != required for name, _ in axes)):
        raise ValueError(f"{flag}: no {required + ' ' if required else ''}{noun} given")
    return axes


def grid_rows(axes: Sequence[Tuple[str, List]], nominal: Dict) -> List[Dict]:
    """The cross product of `parse_axis_grid`'s axes, in itertools.product order of the axes as written (the last axis varies fastest): per
    combination `nominal` with the named axes replaced."""
    return [dict(nominal, **{name: v for (name, _), v in zip(axes, combo)}) for combo in itertools.product(*[vals for _, vals in axes])]


def parse_key_values(flag: str, spec: str, nominal: Dict, noun: str, value: Callable) -> Dict:
    """`KEY=V[,KEY=V...]` -> `nominal` with the named keys replaced by `value(flag, key, text)`, which raises for an unknown key or a value
    the flag does not take.  ValueError, as `flag`'s, for a part without `=`, a key (a `noun`: "axis" or "key") given twice and a spec
    that names none."""
    out, seen = dict(nominal), []
    for part in str(spec).split(","):
        part = part.strip()
        if not part:
            continue
        name, eq, text = part.partition("=")
        name = name.strip()
        if not eq:
            raise ValueError(f"{flag}: {part!r} is not KEY=VALUE")
        if name in seen:
            raise ValueError(f"{flag}: {noun} {name!r} given twice")
        out[name] = value(flag, name, text.strip())      # (an unknown key is refused before it is stored)
        seen.append(name)
    if not seen:
        raise ValueError(f"{flag}: no {noun} given")
    return out


def cell_rows(per_cell, ncommands: int, envs_per_cell: int) -> np.ndarray:
    """The one layout of every sweep: command blocks outermost, cell (c, p) of P cells per command drives envs (c * P + p) * envs_per_cell
    onwards.  `per_cell` ([P] or [P, k], a row per cell) -> the row of every env ([ncommands * P * envs_per_cell(, k)])."""
    per_cell = np.asarray(per_cell)
    return np.tile(np.repeat(per_cell, int(envs_per_cell), axis=0), (int(ncommands),) + (1,) * (per_cell.ndim - 1))
