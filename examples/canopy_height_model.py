"""Rasters on the device: the scene of examples/height_above_ground.py -> progressive morphological filter -> LAS class 2 -> a terrain model,
a surface model and a canopy (object) height model on the ground filter's grid, holes filled, with the tallest canopy cell over each object
next to the height it was built with.

What a PDAL user writes as filters.pmf + filters.hag_nn + writers.gdal (output_type max, window_size 2).  Only the rasters leave the device.  Usage:

    python examples/canopy_height_model.py [terrain points]
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

_spec = importlib.util.spec_from_file_location("classify_ground_scene", os.path.join(ROOT, "examples", "classify_ground.py"))
scene_module = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scene_module)

CELL = 1.0  # metres
FILL = 2    # cells: writers.gdal's window_size


def main(n_terrain=200_000):
    pts, owner = scene_module.scene(n_terrain)
    n = len(pts)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    params = pa.PmfParameters(cell_size=CELL, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)

    # 1. the ground: LAS class 2, then the mask of the ground points and the mask of the finite points that are not ground
    n_ground = pa.classify_ground(cloud, params)
    ground, other = _DeviceArray(cloud.api, T.U8, n), _DeviceArray(cloud.api, T.U8, n)
    pa.classification_mask(cloud, 2, ground.ptr)
    pa.algorithms.finite_mask(cloud, other.ptr)
    pa.algorithms.set_u8_where(other.buffer, other.attribute, ground.ptr, 0)
    grid = pa.pmf_grid(cloud, CELL)  # the grid every raster below is laid on
    (x0, y0), cols, rows = grid["origin"], grid["cols"], grid["rows"]
    print(f"{n} points, {n_ground} on the ground; rasters of {cols} x {rows} cells of {CELL} m")

    # 2. the terrain model: the ground elevation under every cell centre, from its 10 nearest ground points
    cx, cy = np.meshgrid(x0 + (np.arange(cols) + 0.5) * CELL, y0 + (np.arange(rows) + 0.5) * CELL)
    centres = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    centres.resize(cols * rows)
    centres.set_attribute_range(A.POSITION_3D, range(0, cols * rows), np.column_stack([cx.ravel(), cy.ravel(), np.zeros(cols * rows)]))
    terrain = pa.height_above_ground(centres, ground.ptr, k=10, ground=cloud, return_ground_z=True)[1].reshape(rows, cols)

    # 3. the surface model: the highest z per cell, holes filled
    raw, filled = _DeviceArray(cloud.api, T.F64, cols * rows), _DeviceArray(cloud.api, T.F64, cols * rows)
    surface_info = pa.rasterize(cloud, CELL, ("max",), device_out_ptr=raw.ptr)
    pa.grid_fill(raw.ptr, filled.ptr, cols, rows, FILL)
    surface_holes = int(np.isnan(raw.to_numpy()).sum())
    surface = filled.to_numpy().reshape(rows, cols).copy()

    # 4. the canopy model: the highest height above ground per cell over the points that are not ground, holes filled
    hag = _DeviceArray(cloud.api, T.F64, n)
    info = pa.height_above_ground_device(cloud, ground.ptr, k=10, hag_ptr=hag.ptr)
    canopy_info = pa.rasterize(cloud, CELL, ("max",), values=hag.ptr, device_mask_ptr=other.ptr, device_out_ptr=raw.ptr)
    pa.grid_fill(raw.ptr, filled.ptr, cols, rows, FILL)
    canopy = filled.to_numpy().reshape(rows, cols).copy()
    assert (surface_info.cols, surface_info.rows, canopy_info.cols, canopy_info.rows) == (cols, rows, cols, rows)  # one grid, whatever the mask
    print(f"surface model: {surface_info.n_members} points, {surface_holes} empty cells before the fill; canopy model: {canopy_info.n_members} points above the ground, "
          f"{int(np.isfinite(canopy).sum())} cells after the fill")

    # 5. the tallest canopy cell over each object, and how far the canopy model is from surface model - terrain model
    found = []
    for k, (ox, oy, sx, sy, h) in enumerate(scene_module.OBJECTS):
        c0, c1 = int((ox - sx / 2 - x0) / CELL), int((ox + sx / 2 - x0) / CELL)
        r0, r1 = int((oy - sy / 2 - y0) / CELL), int((oy + sy / 2 - y0) / CELL)
        tallest = float(np.nanmax(canopy[r0:r1 + 1, c0:c1 + 1]))
        built = scene_module.CLEAR + h
        found.append({"object": k, "tallest": tallest, "built": built})
        print(f"  object {k} at ({ox:.1f}, {oy:.1f}): tallest canopy cell {tallest:.2f} m; built {built:.2f} m above the terrain")
    both = np.isfinite(canopy) & np.isfinite(surface) & np.isfinite(terrain)
    largest = float(np.abs((surface - terrain) - canopy)[both].max())
    print(f"largest |(surface - terrain) - canopy| over the {int(both.sum())} cells that have all three: {largest:.2f} m")
    return {"found": found, "largest_difference": largest, "n_unresolved": info["n_unresolved"], "cols": cols, "rows": rows, "surface_members": surface_info.n_members,
            "n_points": n}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
