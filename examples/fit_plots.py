#!/usr/bin/env python3
"""The pictures PopPUNK draws at the end of --create-db and --fit-model, from a matrix that never leaves the device:

  resident (core, accessory) matrix of a synthetic database      engine.dist
    -> plot.plot_scatter: the distance distribution under the contours of its kernel density, every row read once
       on the device (engine.density_kde_dev)                                    PopPUNK/plot.py:31-82
    -> BGMMModel.fit_dev, assign_dev                                             PopPUNK/models.py:305-338
    -> BGMMModel.plot: the rows coloured by component with the components' ellipses, and the likelihood surface
       with the within / between boundary                                        PopPUNK/plot.py:182-235, :375-414
  Above `raster_above` rows the scatter layers are one image of the per-label occupancy raster
  (engine.density_counts_dev) instead of one marker per row.

    python examples/fit_plots.py [n_genomes] [strain_size] [raster_above] [workdir]      # needs an MI355X and matplotlib
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppunk_amd import engine, models, plot, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    strain = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    raster_above = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
    work = sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix="ppk_plots_")
    out = os.path.join(work, "synthetic")
    os.makedirs(out, exist_ok=True)
    kmers = np.asarray(synth.DEFAULT_KMERS, dtype=np.int32)
    sketches, _ = synth.make_sketches(n, kmers, cluster_size=strain, seed=7)
    db = engine.SketchDB(sketches, 16, 14, device=0)
    dist_t, _ = engine.dist(db, None, kmers, synth.random_match_table(kmers))
    db.close()
    rows = int(dist_t.shape[0])
    print("distances: %d pairs resident on the device; the scatter layers are drawn as %s"
          % (rows, "rasters" if rows > raster_above else "points"))

    sd = plot.scatter_density(dist_t)
    print("kernel density of all %d rows on the 100 x 100 grid: scale %s, peak %.4g, fixed-point shift %d"
          % (sd.rows_read, sd.scale, sd.z.max(), sd.shift))
    plot.plot_scatter(dist_t, out, "synthetic distances", raster_above=raster_above)

    model = models.BGMMModel.fit_dev(dist_t, 2, max_samples=None, seed=42)
    y = model.assign_dev(dist_t)
    model.plot(dist_t, y, outPrefix=out, raster_above=raster_above)
    for name in ("synthetic_distanceDistribution.png", "synthetic_DPGMM_fit.png", "synthetic_DPGMM_fit_contours.pdf"):
        path = os.path.join(out, name)
        print("%s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
