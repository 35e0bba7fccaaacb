"""include/botlab/obstacle_tracks.hpp and MotionPlannerT::setMapWithTracks compile as a C++11 host translation unit
(tests/cpp/check_obstacle_tracks.cpp, syntax only, with the struct sizes and offsets asserted), and the structs of the Python binding
have the header's layout."""
import ctypes
import os
import subprocess

import numpy as np

from botlab_amd import _capi
import obstacle_tracks_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles():
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "check_obstacle_tracks.cpp")])


def _offsets(s):
    return tuple(getattr(s, name).offset for name, _ in s._fields_)


def test_struct_layouts():
    assert ctypes.sizeof(_capi.ObsTracksParams) == 32 and _offsets(_capi.ObsTracksParams) == (0, 4, 8, 12, 16, 20, 24, 28)
    assert ctypes.sizeof(_capi.ObsTracksCompose) == 16 and _offsets(_capi.ObsTracksCompose) == (0, 4, 8, 12)
    assert ctypes.sizeof(_capi.ObsTrack) == 56 and _offsets(_capi.ObsTrack) == tuple(range(0, 56, 4))
    assert ctypes.sizeof(_capi.ObsBlob) == 56 and _offsets(_capi.ObsBlob) == (0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52)
    assert ctypes.sizeof(_capi.ObsTracksStats) == 56 and _offsets(_capi.ObsTracksStats) == tuple(range(0, 56, 4))
    assert ctypes.sizeof(_capi.ObsTracksState) == 16 and _offsets(_capi.ObsTracksState) == (0, 4, 8, 12)
    # the numpy records of the host and of the model are those structs
    for dtype, struct in ((np.dtype(_capi.OBSTRACK_DTYPE), _capi.ObsTrack), (np.dtype(_capi.OBSBLOB_DTYPE), _capi.ObsBlob)):
        assert dtype.itemsize == ctypes.sizeof(struct) and tuple(dtype.names) == tuple(n for n, _ in struct._fields_)
        assert tuple(dtype.fields[n][1] for n in dtype.names) == _offsets(struct)
    assert np.dtype(_capi.OBSTRACK_DTYPE) == tm.TRACK_DTYPE and np.dtype(_capi.OBSBLOB_DTYPE) == tm.BLOB_DTYPE
    assert tuple(n for n, _ in _capi.ObsTracksStats._fields_) == tm.STAT_NAMES
    assert tuple(n for n, _ in _capi.ObsTracksParams._fields_) == tm.PARAM_NAMES


def test_header_states_the_layout_the_binding_has():
    text = open(os.path.join(ROOT, "include", "botlab_hip.h")).read()
    for line in ("32 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28", "16 bytes: offsets 0, 4, 8, 12",
                 "56 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52", "56 bytes: offsets 0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52"):
        assert line in text, line
    for name in ("bl_obstracks_create", "bl_obstracks_update", "bl_obstracks_compose", "bl_obstracks_tracks", "bl_obstracks_blobs",
                 "bl_obstracks_labels", "bl_obstracks_stats", "bl_obstracks_download", "bl_obstracks_upload", "bl_obstracks_reset",
                 "bl_obstracks_last_device_ms"):
        assert name in _capi.SIGNATURES
