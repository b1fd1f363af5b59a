"""numpy fp64 restatement of the catchment-forcing rule
(tfg_set_catchment_forcing, csrc/tfg_forcing.hpp): what the kernel is pinned
to.  Test infrastructure; the reference has no such term (one cell per
catchment).

For cell i with c = catch_id[i] (0 without a raster), dz = elev[i] - z_ref[c]
and X_c the table value of catchment c for the frame:
  uz     = uz_c
  T_air  = T_c + lapse_T dz
  P      = P_c max(0, 1 + grad_P dz)
  P_air  = P_air_c exp(-M g dz / (R (T_c + 273.15)))       when pressure == 1
  Hum_sp = q_c; with rh_max > 0, where e = q P_air / (eps + (1 - eps) q) / 100
           exceeds e_cap = rh_max e_sat(T_air):
           q = eps e_cap / (P_air / 100 - (1 - eps) e_cap)
with e_sat the model's configured form in mbar (the oracle's _e_sat, :747-807).
"""

from __future__ import annotations

import numpy as np

import tfg_oracle as O

ORDER = ("P_air", "Hum_sp", "P", "T_air", "uz")  # tfg_set_inputs order: axis 1 of a table and of the result
I_PA, I_Q, I_P, I_T, I_UZ = range(5)
OFF = dict(lapse_T=0.0, grad_P=0.0, pressure=0, rh_max=0.0)


def constants(cfg: dict | None = None) -> dict:
    c = dict(O.CFG_DEFAULTS)
    c.update(cfg or {})
    return c


def e_sat(T, c: dict):
    """Saturation vapour pressure [mbar] (tfg_oracle.OracleGrid._e_sat)."""
    T = np.asarray(T, dtype=np.float64)
    if not c["SATTERLUND"]:
        e = np.float64(0.611) * np.exp((np.float64(17.3) * T) / (T + np.float64(237.3)))
    else:
        e = np.float64(10) ** (np.float64(11.4) - np.float64(2353) / (T + np.float64(273.15))) / np.float64(1000)
    return e * np.float64(10)


def vapour_pressure(q, P_air, c: dict):
    """e [mbar] of a specific humidity (:809-826)."""
    eps = np.float64(c["eps"])
    return q * P_air / (eps + (1 - eps) * q) / np.float64(100)


def relative_humidity(frames, c: dict):
    """RH the model computes from frames [..., 5, ncell] (:828-838)."""
    return vapour_pressure(frames[..., I_Q, :], frames[..., I_PA, :], c) / e_sat(frames[..., I_T, :], c)


def downscale(table, cid, elev=None, z_ref=None, lapse_T=0.0, grad_P=0.0, pressure=0, rh_max=0.0, cfg: dict | None = None,
              parts: bool = False):
    """[nframes][5][ncell] fp64 frames in tfg_set_inputs order from a table
    [nframes][5][n_catch], the id per cell (None: all 0, `elev` then gives the
    cell count), the elevation per cell as the engine holds it and z_ref
    [n_catch].  parts=True also returns dict(dz, clamped [ncell], rh_before
    [nframes][ncell]: the RH of the uncapped humidity)."""
    table = np.asarray(table, dtype=np.float64)
    if cid is None:
        cid = np.zeros(np.asarray(elev).size, dtype=np.int64)
    cid = np.asarray(cid).reshape(-1)
    out = table[:, :, cid].copy()  # the plain gather
    on = lapse_T != 0.0 or grad_P != 0.0 or pressure == 1 or rh_max > 0.0
    if not on:
        return (out, {}) if parts else out
    c = constants(cfg)
    dz = np.asarray(elev, dtype=np.float64).reshape(-1) - np.asarray(z_ref, dtype=np.float64)[cid]
    T_c = out[:, I_T, :].copy()
    fac = 1.0 + np.float64(grad_P) * dz
    out[:, I_T, :] = T_c + np.float64(lapse_T) * dz
    out[:, I_P, :] = out[:, I_P, :] * np.maximum(0.0, fac)
    if pressure == 1:
        x = -np.float64(c["M_mass_air"]) * np.float64(c["g"]) * dz / (np.float64(c["uni_gas_const"]) * (T_c + 273.15))
        out[:, I_PA, :] = out[:, I_PA, :] * np.exp(x)
    info = {"dz": dz, "clamped": fac <= 0.0, "rh_before": relative_humidity(out, c)}
    if rh_max > 0.0:
        eps = np.float64(c["eps"])
        q, pa = out[:, I_Q, :], out[:, I_PA, :]
        e = vapour_pressure(q, pa, c)
        e_cap = np.float64(rh_max) * e_sat(out[:, I_T, :], c)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, I_Q, :] = np.where(e > e_cap, eps * e_cap / (pa / np.float64(100) - (1 - eps) * e_cap), q)
    return (out, info) if parts else out


def catchment_means(cid, values, n_catch: int):
    """[..., n_catch] mean of values [..., ncell] over each catchment's cells (0 without cells)."""
    cid = np.asarray(cid).reshape(-1)
    v = np.asarray(values, dtype=np.float64)
    cells = np.bincount(cid, minlength=n_catch)
    flat = v.reshape(-1, cid.size)
    sums = np.stack([np.bincount(cid, weights=row, minlength=n_catch) for row in flat])
    return (np.where(cells > 0, sums / np.maximum(cells, 1), 0.0)).reshape(v.shape[:-1] + (n_catch,))
