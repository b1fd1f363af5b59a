"""Forcing ingestion for the callers of the melt update.

The reference feeds one catchment per step from a NextGen forcing CSV in its
example driver (examples/run_topoflow_glacier.py:30-73).  This module is that
mapping, column for column and with the same unit conversions in the same
operation order, so the values a caller hands to ``set_value`` are bit-identical
to the reference driver's:

  BMI input (_dynamic_input_vars, bmi_topoflow_glacier.py:18-26)   CSV column(s)
  atmosphere_water__liquid_equivalent_precipitation_rate            RAINRATE * 10**(-3)   (mm/h -> m/h, :64-65)
  land_surface_air__temperature                                     K_to_C + T2D          (K -> degC, :66)
  land_surface_radiation~incoming~longwave__energy_flux              LWDOWN                (:67)
  land_surface_radiation~incoming~shortwave__energy_flux             SWDOWN                (:68)
  land_surface_air__pressure                                        PSFC                  (:69)
  atmosphere_air_water~vapor__relative_saturation                   Q2D (specific humidity, :70)
  wind_speed_UV                                                     ((U2D)**2 + (V2D)**2)**0.5  (:45-47)

Rows are selected by ``start_time <= Time <= end_time`` (:33-40).  For grids,
:func:`frames_from_table` broadcasts or stacks per-cell tables into the
``[nsteps][ncell]`` frame arrays :meth:`GlacierEngine.set_field` uploads.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

__all__ = ["BMI_INPUTS", "INTERNAL", "K_TO_C", "ForcingTable", "read_forcing_csv", "frames_from_table",
           "INPUT_ORDER", "Downscale", "catchment_table", "ForcingGrid"]

K_TO_C = -273.15  # BmiTopoflowGlacier.K_to_C (bmi_topoflow_glacier.py:290)

# BMI input name -> internal name (the engine's field names, _native.FIELD)
BMI_INPUTS = {
    "land_surface_radiation~incoming~longwave__energy_flux": "LW_in",
    "land_surface_air__pressure": "P_air",
    "atmosphere_air_water~vapor__relative_saturation": "Hum_sp",
    "atmosphere_water__liquid_equivalent_precipitation_rate": "P",
    "land_surface_radiation~incoming~shortwave__energy_flux": "SW_in",
    "land_surface_air__temperature": "T_air",
    "wind_speed_UV": "uz",
}
INTERNAL = {v: k for k, v in BMI_INPUTS.items()}


@dataclass
class ForcingTable:
    """Per-step BMI inputs of one catchment (float64, reference units)."""

    times: np.ndarray                      # datetime64[ns], one per step
    inputs: dict = field(default_factory=dict)  # internal name -> [nsteps] float64

    def __len__(self) -> int:
        return len(self.times)

    def step(self, i: int) -> dict:
        """BMI name -> value of step i (what the reference driver set_value()s)."""
        return {INTERNAL[k]: v[i] for k, v in self.inputs.items()}

    def apply(self, model, i: int) -> None:
        """set_value() every input of step i on a BMI model (:63-71)."""
        for name, value in self.step(i).items():
            model.set_value(name, value)


def read_forcing_csv(path: str | Path, start_time: str | None = None, end_time: str | None = None) -> ForcingTable:
    """Read a NextGen forcing CSV (columns Time, RAINRATE, T2D, LWDOWN, SWDOWN,
    PSFC, Q2D, U2D, V2D) between start_time and end_time (YYYYmmddHH, inclusive)."""
    import pandas as pd

    df = pd.read_csv(path)
    missing = {"Time", "RAINRATE", "T2D", "LWDOWN", "SWDOWN", "PSFC", "Q2D", "U2D", "V2D"} - set(df.columns)
    if missing:
        raise KeyError(f"{path}: forcing columns missing: {sorted(missing)}")
    df["Time"] = pd.to_datetime(df["Time"])
    if start_time is not None:
        df = df[df["Time"] >= pd.to_datetime(str(start_time), format="%Y%m%d%H")]
    if end_time is not None:
        df = df[df["Time"] <= pd.to_datetime(str(end_time), format="%Y%m%d%H")]
    df = df.copy()
    wind = (((df["U2D"]) ** 2 + (df["V2D"]) ** 2) ** 0.5).values
    inputs = {
        "P": df["RAINRATE"].values * 10 ** (-3),
        "T_air": K_TO_C + df["T2D"].values,
        "LW_in": df["LWDOWN"].values.astype(np.float64),
        "SW_in": df["SWDOWN"].values.astype(np.float64),
        "P_air": df["PSFC"].values.astype(np.float64),
        "Hum_sp": df["Q2D"].values.astype(np.float64),
        "uz": wind,
    }
    return ForcingTable(times=df["Time"].values, inputs={k: np.asarray(v, dtype=np.float64) for k, v in inputs.items()})


def frames_from_table(table: ForcingTable, ncell: int = 1) -> dict:
    """internal name -> [nsteps][ncell] frames (the table broadcast to ncell cells)."""
    return {k: np.ascontiguousarray(np.broadcast_to(v[:, None], (len(v), ncell))) for k, v in table.inputs.items()}


INPUT_ORDER = ("P_air", "Hum_sp", "P", "T_air", "uz")  # tfg_set_inputs order: the five inputs the physics reads


@dataclass
class Downscale:
    """Elevation terms of GlacierEngine.set_catchment_forcing (tfg_downscale),
    every one off by default.  With dz = a cell's elevation minus its
    catchment's reference elevation:

      lapse_T   T_air = T_c + lapse_T dz                       [degC m-1], e.g. -0.0065
      grad_P    P = P_c max(0, 1 + grad_P dz)                  [m-1]
      pressure  1: P_air = P_air_c exp(-M g dz / (R (T_c + 273.15)))
      rh_max    > 0: Hum_sp capped so that the cell's relative humidity stays
                at or under rh_max (1.0 = saturation)
    """

    lapse_T: float = 0.0
    grad_P: float = 0.0
    pressure: int = 0
    rh_max: float = 0.0

    @property
    def on(self) -> bool:
        return bool(self.lapse_T != 0.0 or self.grad_P != 0.0 or self.pressure == 1 or self.rh_max > 0.0)


def catchment_table(tables) -> np.ndarray:
    """[nsteps][5][n_catch] float64 in tfg_set_inputs order (P_air, Hum_sp, P,
    T_air, uz) from one ForcingTable per catchment, in catchment-id order: what
    GlacierEngine.set_catchment_forcing spreads over the grid.  The tables
    must cover the same steps: equal lengths and equal times."""
    tables = list(tables)
    if not tables:
        raise ValueError("catchment_table: no tables")
    n = len(tables[0])
    for c, t in enumerate(tables):
        if len(t) != n:
            raise ValueError(f"catchment_table: catchment {c} has {len(t)} steps, catchment 0 has {n}")
        if not np.array_equal(np.asarray(t.times), np.asarray(tables[0].times)):
            raise ValueError(f"catchment_table: the times of catchment {c} differ from catchment 0's")
    out = np.empty((n, 5, len(tables)), dtype=np.float64)
    for c, t in enumerate(tables):
        for v, name in enumerate(INPUT_ORDER):
            out[:, v, c] = t.inputs[name]
    return out


def _axis_map(src, first: float, step: float, name: str):
    """(origin, scale) of one axis: the source-grid coordinate (node j at j) of
    model cell k is origin + scale k, from the nodes' coordinates `src` and
    the cell centres first + step k."""
    src = np.asarray(src, dtype=np.float64).reshape(-1)
    if src.size < 1 or not np.isfinite(src).all():
        raise ValueError(f"ForcingGrid.from_axes: {name} needs at least one finite node coordinate")
    if src.size == 1:  # one node: every coordinate clamps to it
        return 0.0, 0.0
    h = (src[-1] - src[0]) / (src.size - 1)
    if h == 0.0 or np.abs(np.diff(src) - h).max() > 1e-6 * abs(h):
        raise ValueError(f"ForcingGrid.from_axes: {name} is not uniformly spaced")
    return float((first - src[0]) / h), float(step / h)


@dataclass
class ForcingGrid:
    """A regular source grid under GlacierEngine.set_gridded_forcing
    (tfg_forcing_grid): gny x gnx nodes, node (j, i) at source-grid coordinate
    (j, i).  The centre of the GLOBAL model cell (row R, column c) sits at the
    source-grid coordinate (y0 + sy R, x0 + sx c); a negative sy or sx is a
    source axis that runs against the model's.  Outside the source grid the
    edge value is held.  method: "bilinear" or "nearest" (ties go up)."""

    gny: int
    gnx: int
    y0: float = 0.0
    x0: float = 0.0
    sy: float = 1.0
    sx: float = 1.0
    method: str = "bilinear"

    METHODS = ("nearest", "bilinear")  # include/tfg.h TFG_REGRID_*

    @classmethod
    def from_axes(cls, src_y, src_x, y_first: float, x_first: float, dy: float, dx: float,
                  method: str = "bilinear") -> "ForcingGrid":
        """The affine map from the source nodes' coordinates src_y [gny] and
        src_x [gnx] (uniformly spaced, ascending or descending, in the model
        grid's coordinate system) and the model grid: the centre of its cell
        (row 0, column 0) at (y_first, x_first), rows dy and columns dx apart
        (signed: dy < 0 for rows that run north to south).  Raises ValueError
        on an axis that is not uniformly spaced."""
        y0, sy = _axis_map(src_y, float(y_first), float(dy), "src_y")
        x0, sx = _axis_map(src_x, float(x_first), float(dx), "src_x")
        return cls(gny=int(np.size(src_y)), gnx=int(np.size(src_x)), y0=y0, x0=x0, sy=sy, sx=sx, method=method)
