"""Generates tests/golden/refmath_erfinv_quantile.npz from oracle/_ref/libradarays_refmath.so -- the reference's own
include/radarays_ros/radar_math.h compiled as-is by `make -C oracle ref` (dev container only: it needs the reference
checkout; what is committed are the header's OUTPUTS beside the inputs they belong to, never the header).

    python -c "from oracle import oracle as O; O.build()" && python tests/golden/gen_refmath.py

refmath_erfinv_quantile.npz
    erfinv_x  [4006] f32  inputs of erfinvf: 4001 points on [-0.999, 0.999] and 0, +-1e-8, +-0.9999
    erfinv_y  [4006] f32  radarays_ros::erfinvf(erfinv_x)
    quantile_p [999] f32  inputs of quantile: 999 points on [0.001, 0.999]
    quantile_y [999] f32  radarays_ros::quantile(quantile_p)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import oracle as O  # noqa: E402

R = O.ref_lib()
if R is None:
    raise SystemExit("oracle/_ref/libradarays_refmath.so is not built (it needs the reference checkout)")
xs = np.concatenate([np.linspace(-0.999, 0.999, 4001), [0.0, 1e-8, -1e-8, 0.9999, -0.9999]]).astype(np.float32)
ps = np.linspace(0.001, 0.999, 999).astype(np.float32)
np.savez(os.path.join(HERE, "refmath_erfinv_quantile.npz"),
         erfinv_x=xs, erfinv_y=np.array([R.ref_erfinvf(float(x)) for x in xs], np.float32),
         quantile_p=ps, quantile_y=np.array([R.ref_quantile(float(p)) for p in ps], np.float32))
