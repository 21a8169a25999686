"""The switch of the bright-tile kernel (k_s2_bright, wfs_tilegen.h) on its way from the fax config to the library: config key
'tile_local_bright' -> kernel_params -> Engine -> wfs_set_bright_tiles.  (What the kernel computes: tests/test_gpu_bright_tiles.py.)"""
import os
import re

from wfsim_amd import engine
from wfsim_amd.config import kernel_params, xenonnt_test_config


def test_tile_local_bright_reaches_the_engine_configuration():
    assert kernel_params(xenonnt_test_config())['tile_local_bright'] == 1          # default: on
    assert kernel_params(xenonnt_test_config(tile_local_bright=False))['tile_local_bright'] == 0
    assert kernel_params(xenonnt_test_config(tile_local_bright=True))['tile_local_bright'] == 1
    # it travels through a setter of its own, not through wfs_config: the struct keeps its layout
    assert 'tile_local_bright' not in [n for n, _ in engine.WfsConfig._fields_]
    header = open(os.path.join(os.path.dirname(engine.HERE), 'include', 'wfsim_amd.h')).read()
    for name in ('wfs_set_bright_tiles', 'wfs_copy_tile_kernels'):
        assert name in engine.EXPORTS and re.search(r'\bint\s+' + name + r'\s*\(', header)
    assert callable(engine.Engine.tile_kernels)
