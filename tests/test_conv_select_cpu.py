"""The kernel-selection rule and the level scheduler both plan builders call (include/idh_ops.h: idh_conv_select, idh_schedule_ops;
csrc/plan_select.hip).  Host only: nothing here touches a device."""
import ctypes as C

import pytest

# The choice for every distinct conv of the shipped networks - CVEncoder(64 -> [64, 128, 256, 384]) + BDDecoderPP / DepthDecoderPP at a 96x128
# cost volume, the matching head over 8 images per frame and layer1 of its stem - at B = 1, 4, 32 frames under the default tuning, recorded from
# nhwc.Plan.conv before the rule moved into the library.  A retune shows up here as a diff.
LAYERS = {
    '1x1/1 64 > 128 @96x128 cs128': ((8, 96, 128, 128, 0, 0, 0.2, 128, 0, 0, 0, 0, ((96, 128, 64, 64, 1, 1),)),
        {1: (4, 4, 1, 0, 0), 4: (4, 4, 1, 0, 0), 32: (4, 4, 1, 0, 0)}),
    '3x3/1 112 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 112, 112, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 + 1x1/1 192 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1), (48, 64, 192, 192, 1, 1))),
        {1: (9, 2, 2, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 + 1x1/1 256 > 128 @24x32 cs128': ((1, 24, 32, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((24, 32, 128, 128, 3, 1), (24, 32, 256, 256, 1, 1))),
        {1: (9, 2, 2, 0, 8), 4: (9, 2, 2, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 128 + 1x1/1 256 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1), (48, 64, 256, 256, 1, 1))),
        {1: (9, 2, 2, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 + 1x1/1 384 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1), (48, 64, 384, 384, 1, 1))),
        {1: (9, 2, 3, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 + 3x3/2 64 > 128 @48x64 cs192': ((1, 48, 64, 128, 0, 1, 0.2, 192, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1), (96, 128, 64, 64, 3, 2))),
        {1: (9, 2, 2, 0, 8), 4: (9, 0, 2, 0, 8), 32: (8, 0, 1, 0, 8)}),
    '3x3/1 128 > 128 @48x64 +res cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 128, 1, 0, 0, ((48, 64, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 > 128 @48x64 +res cs256': ((1, 48, 64, 128, 0, 1, 0.2, 256, 128, 1, 0, 0, ((48, 64, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 > 128 @48x64 +res cs384': ((1, 48, 64, 128, 0, 1, 0.2, 384, 128, 1, 0, 0, ((48, 64, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 > 16 @96x128 norm rep cs16': ((8, 96, 128, 16, 1, 0, 0.2, 16, 0, 0, 1, 0, ((96, 128, 128, 128, 3, 1),)),
        {1: (8, 1, 1, 0, 8), 4: (8, 1, 1, 0, 8), 32: (8, 1, 1, 0, 8)}),
    '3x3/1 128 > 16 @96x128 rep cs16': ((8, 96, 128, 16, 1, 0, 0.2, 16, 0, 0, 0, 0, ((96, 128, 128, 128, 3, 1),)),
        {1: (8, 1, 1, 0, 8), 4: (8, 1, 1, 0, 8), 32: (8, 1, 1, 0, 8)}),
    '3x3/1 128 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 128, 128, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 128 > 64 @48x64 cs64': ((1, 48, 64, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (9, 2, 1, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 128 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 128, 128, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 192 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 192, 192, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 192 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 192, 192, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 192 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 192, 192, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 24 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 32, 24, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 256 + 1x1/1 384 > 256 @12x16 cs256': ((1, 12, 16, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((12, 16, 256, 256, 3, 1), (12, 16, 384, 384, 1, 1))),
        {1: (9, 2, 4, 0, 8), 4: (9, 2, 4, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/1 256 + 1x1/1 416 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 1), (24, 32, 416, 416, 1, 1))),
        {1: (9, 2, 4, 0, 8), 4: (9, 0, 4, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 256 + 1x1/1 512 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 1), (24, 32, 512, 512, 1, 1))),
        {1: (9, 2, 5, 0, 8), 4: (9, 0, 4, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 256 + 3x3/2 128 > 256 @24x32 cs416': ((1, 24, 32, 256, 0, 1, 0.2, 416, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 1), (48, 64, 128, 128, 3, 2))),
        {1: (9, 2, 4, 0, 8), 4: (9, 0, 4, 0, 8), 32: (8, 0, 1, 0, 8)}),
    '3x3/1 256 > 128 @24x32 cs128': ((1, 24, 32, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (9, 2, 2, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 256 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 256, 256, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 256 > 256 @24x32 +res cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 256, 1, 0, 0, ((24, 32, 256, 256, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (9, 2, 2, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 256 > 256 @24x32 +res cs512': ((1, 24, 32, 256, 0, 1, 0.2, 512, 256, 1, 0, 0, ((24, 32, 256, 256, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (9, 2, 2, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 256 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 1),)),
        {1: (9, 2, 2, 0, 8), 4: (9, 2, 2, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 384 + 1x1/1 640 > 384 @12x16 cs384': ((1, 12, 16, 384, 0, 1, 0.2, 384, 0, 0, 0, 0, ((12, 16, 384, 384, 3, 1), (12, 16, 640, 640, 1, 1))),
        {1: (9, 2, 7, 0, 8), 4: (9, 0, 7, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/1 384 + 3x3/2 256 > 384 @12x16 cs640': ((1, 12, 16, 384, 0, 1, 0.2, 640, 0, 0, 0, 0, ((12, 16, 384, 384, 3, 1), (24, 32, 256, 256, 3, 2))),
        {1: (9, 2, 6, 0, 8), 4: (9, 0, 6, 0, 8), 32: (9, 0, 2, 0, 8)}),
    '3x3/1 384 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((48, 64, 384, 384, 3, 1),)),
        {1: (9, 2, 4, 0, 8), 4: (12, 0, 1, 1, 9), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 384 > 256 @12x16 cs256': ((1, 12, 16, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((12, 16, 384, 384, 3, 1),)),
        {1: (9, 2, 4, 0, 8), 4: (9, 2, 4, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/1 384 > 384 @12x16 +res cs384': ((1, 12, 16, 384, 0, 1, 0.2, 384, 384, 1, 0, 0, ((12, 16, 384, 384, 3, 1),)),
        {1: (9, 2, 4, 0, 8), 4: (9, 2, 4, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/1 384 > 384 @12x16 cs384': ((1, 12, 16, 384, 0, 1, 0.2, 384, 0, 0, 0, 0, ((12, 16, 384, 384, 3, 1),)),
        {1: (9, 2, 4, 0, 8), 4: (9, 2, 4, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/1 416 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((24, 32, 416, 416, 3, 1),)),
        {1: (9, 2, 4, 0, 8), 4: (9, 0, 4, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 512 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((24, 32, 512, 512, 3, 1),)),
        {1: (9, 2, 5, 0, 8), 4: (9, 0, 4, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 64 + 1x1/1 112 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 64, 64, 3, 1), (96, 128, 112, 112, 1, 1))),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 + 1x1/1 128 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 64, 64, 3, 1), (192, 256, 128, 128, 1, 1))),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 + 1x1/1 128 > 64 @48x64 cs64': ((1, 48, 64, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((48, 64, 64, 64, 3, 1), (48, 64, 128, 128, 1, 1))),
        {1: (9, 2, 1, 0, 8), 4: (9, 2, 1, 0, 8), 32: (12, 0, 1, 1, 13)}),
    '3x3/1 64 + 1x1/1 128 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 64, 64, 3, 1), (96, 128, 128, 128, 1, 1))),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 + 1x1/1 192 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 64, 64, 3, 1), (192, 256, 192, 192, 1, 1))),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 + 1x1/1 192 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 64, 64, 3, 1), (96, 128, 192, 192, 1, 1))),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 + 1x1/1 24 > 64 @192x256 cs192': ((1, 192, 256, 64, 0, 1, 0.2, 192, 0, 0, 0, 0, ((192, 256, 64, 64, 3, 1), (192, 256, 32, 24, 1, 1))),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @192x256 +res cs128': ((1, 192, 256, 64, 0, 1, 0.2, 128, 64, 1, 0, 0, ((192, 256, 64, 64, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @192x256 +res cs192': ((1, 192, 256, 64, 0, 1, 0.2, 192, 64, 1, 0, 0, ((192, 256, 64, 64, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @192x256 +res cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 64, 1, 0, 0, ((192, 256, 64, 64, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @192x256 cs64': ((1, 192, 256, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((192, 256, 64, 64, 3, 1),)),
        {1: (12, 0, 1, 1, 13), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 +res any cs64': ((8, 96, 128, 64, 0, 1, 0.0, 64, 64, 1, 0, 1, ((96, 128, 64, 64, 3, 1),)),
        {1: (13, 0, 1, 2, 15), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 +res cs112': ((1, 96, 128, 64, 0, 1, 0.2, 112, 64, 1, 0, 0, ((96, 128, 64, 64, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 +res cs128': ((1, 96, 128, 64, 0, 1, 0.2, 128, 64, 1, 0, 0, ((96, 128, 64, 64, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 +res cs192': ((1, 96, 128, 64, 0, 1, 0.2, 192, 64, 1, 0, 0, ((96, 128, 64, 64, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 +res cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 64, 1, 0, 0, ((96, 128, 64, 64, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 any cs64': ((8, 96, 128, 64, 0, 1, 0.0, 64, 0, 0, 0, 1, ((96, 128, 64, 64, 3, 1),)),
        {1: (13, 0, 1, 2, 15), 4: (13, 0, 1, 2, 15), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 64 > 64 @96x128 cs64': ((1, 96, 128, 64, 0, 1, 0.2, 64, 0, 0, 0, 0, ((96, 128, 64, 64, 3, 1),)),
        {1: (9, 2, 1, 0, 8), 4: (12, 0, 1, 1, 13), 32: (13, 0, 1, 2, 15)}),
    '3x3/1 640 > 384 @12x16 cs384': ((1, 12, 16, 384, 0, 1, 0.2, 384, 0, 0, 0, 0, ((12, 16, 640, 640, 3, 1),)),
        {1: (9, 2, 6, 0, 8), 4: (9, 0, 6, 0, 8), 32: (9, 0, 2, 0, 12)}),
    '3x3/2 128 > 256 @24x32 cs256': ((1, 24, 32, 256, 0, 1, 0.2, 256, 0, 0, 0, 0, ((48, 64, 128, 128, 3, 2),)),
        {1: (1, 4, 6, 0, 0), 4: (1, 4, 2, 0, 0), 32: (8, 0, 1, 0, 16)}),
    '3x3/2 256 > 384 @12x16 cs384': ((1, 12, 16, 384, 0, 1, 0.2, 384, 0, 0, 0, 0, ((24, 32, 256, 256, 3, 2),)),
        {1: (1, 4, 15, 0, 0), 4: (1, 4, 4, 0, 0), 32: (9, 0, 2, 0, 16)}),
    '3x3/2 64 > 128 @48x64 cs128': ((1, 48, 64, 128, 0, 1, 0.2, 128, 0, 0, 0, 0, ((96, 128, 64, 64, 3, 2),)),
        {1: (1, 4, 3, 0, 0), 4: (1, 4, 1, 0, 0), 32: (8, 0, 1, 0, 16)}),
}


def _desc(_lib, d, B=1, math=0, cat=False):
    N, Ho, Wo, Cout, pad, act, slope, out_cs, res_cs, has_res, has_norm, any_size, srcs = d
    dd = _lib.ConvDesc(N * B, Ho, Wo, Cout, pad, act, slope, out_cs, res_cs, has_res, has_norm, any_size, math, len(srcs))
    for s, v in zip(dd.src, srcs):
        s.H, s.W, s.cs, s.Cin, s.ks, s.stride = v
        s.is_cat = cat
    return dd


def _select(d, tuning=None, rc=0):
    from implicit_depth_amd import _lib

    ch = _lib.ConvChoice()
    assert _lib.lib().idh_conv_select(C.byref(d) if d is not None else None, C.byref(tuning) if tuning is not None else None, C.byref(ch)) == rc
    return ch


def _answer(ch):
    return (ch.tile_m, ch.tile_n, ch.split_k, ch.w_layout, ch.families)


def test_struct_mirrors_match_the_library():
    from implicit_depth_amd import _lib

    sizes = (C.c_size_t * 3)()
    _lib.lib().idh_sizeof_conv_select(sizes)
    assert list(sizes) == [C.sizeof(_lib.ConvDesc), C.sizeof(_lib.ConvTuning), C.sizeof(_lib.ConvChoice)]


def test_shipped_layers_keep_their_kernels():
    """(a) the table; (b) NULL tuning = the struct built from nhwc's module globals."""
    from implicit_depth_amd import _lib, nhwc

    assert len(LAYERS) == 59
    for name, (d, want) in LAYERS.items():
        for B, w in want.items():
            assert _answer(_select(_desc(_lib, d, B))) == w, (name, B)
            assert _answer(_select(_desc(_lib, d, B), nhwc.conv_tuning())) == w, (name, B)


def _retuned(name, B, math=0, cat=False, **knobs):
    from implicit_depth_amd import _lib, nhwc

    t = nhwc.conv_tuning()
    base = _select(_desc(_lib, LAYERS[name][0], B, math, cat), t)
    for k, v in knobs.items():
        assert hasattr(t, k), k
        setattr(t, k, v)
    return base, _select(_desc(_lib, LAYERS[name][0], B, math, cat), t)


def test_each_knob_moves_a_layer():
    """(c) the overrides tests and tools use, each on a layer it is meant for."""
    W4, W2, SPLIT = 13, 12, 11  # IDH_TILE_WINO4, IDH_TILE_WINO, IDH_SPLIT_F16X3
    full, half, low = "3x3/1 64 > 64 @192x256 +res cs64", "3x3/1 64 > 64 @96x128 +res cs64", "3x3/1 384 > 384 @12x16 +res cs384"
    proj, down = "3x3/1 64 + 1x1/1 192 > 64 @192x256 cs64", "3x3/2 64 > 128 @48x64 cs128"
    b, r = _retuned(full, 1, wino4_min_tiles=1, wino4_min_fill=0)
    assert (b.tile_m, r.tile_m, r.w_layout) == (W2, W4, 2)
    b, r = _retuned(low, 1, wino_min_tiles=1, wino_min_fill=0)
    assert b.tile_m == 9 and (r.tile_m, r.w_layout) == (W2, 1)
    b, r = _retuned(full, 1, winograd=0)
    assert b.tile_m == W2 and r.tile_m in (8, 9) and r.w_layout == 0 and r.families == b.families
    b, r = _retuned(full, 32, winograd4=0)
    assert (b.tile_m, r.tile_m) == (W4, W2)
    b, r = _retuned(proj, 32, winograd4_proj=0)
    assert (b.tile_m, r.tile_m) == (W4, W2) and not r.families & 2
    b, r = _retuned(low, 1, math=SPLIT, split_min_blocks=1)
    assert b.tile_m == 9 and (r.tile_m, r.tile_n, r.w_layout) == (SPLIT, 8, 3)
    b, r = _retuned(down, 1, s2_first_min_blocks=0)
    assert (b.tile_m, b.tile_n) == (1, 4) and r.tile_m == 9 and r.families & 16
    b, r = _retuned(down, 1, s2_first=0, s2_first_min_blocks=0)
    assert (r.tile_m, r.families & 16) == (b.tile_m, 0)
    b, r = _retuned(half, 1, narrow_tile_below=0)  # 192 workgroups of 64 channels: 32-channel tiles unless the rule is off
    assert (b.tile_m, b.tile_n) == (9, 2) and (r.tile_m, r.tile_n) == (9, 0)
    _, b = _retuned(half, 4, winograd=0)  # 768 workgroups: between the shipped threshold and 800
    _, r = _retuned(half, 4, winograd=0, narrow_tile_below=800)
    assert (b.tile_m, b.tile_n) == (9, 0) and (r.tile_m, r.tile_n) == (9, 2)
    b, r = _retuned(low, 1, narrowest_tile_below=100)
    assert (b.tile_m, b.tile_n) == (9, 2) and (r.tile_m, r.tile_n) == (9, 1)
    b, r = _retuned(full, 32, cat=True, fused_up_rows=8)  # a fused-upsample concat source: 4-row tiles unless FUSED_UP_ROWS says 8
    assert (b.tile_m, r.tile_m) == (9, 8) and not b.families & 3


def test_malformed_descriptors_are_refused():
    """(d)"""
    from implicit_depth_amd import _lib

    good = LAYERS["3x3/1 64 + 1x1/1 192 > 64 @192x256 cs64"][0]
    assert _select(_desc(_lib, good)).tile_m == 12

    def bad(**kw):
        d = _desc(_lib, good)
        for k, v in kw.items():
            if k.startswith("src_"):
                setattr(d.src[0], k[4:], v)
            else:
                setattr(d, k, v)
        _select(d, rc=-1)  # IDH_EINVAL

    for n_src in (0, 3, -1):
        bad(n_src=n_src)
    bad(src_ks=2)
    bad(src_ks=0)
    for f in ("N", "Ho", "Wo", "Cout"):
        bad(**{f: 0})
        bad(**{f: -4})
    bad(src_stride=0)
    bad(src_Cin=-16)
    bad(math=5)
    _select(None, rc=-1)
    t = _lib.ConvTuning()
    _lib.lib().idh_conv_tuning_defaults(C.byref(t))
    t.split_min_chunks = 0
    _select(_desc(_lib, good), t, rc=-1)
    assert _lib.lib().idh_conv_select(C.byref(_desc(_lib, good)), None, None) == -1


def test_two_segment_schedule():
    """(e) idh_schedule_ops: levels restart at n_first, the grouped ranks carry level + 1, everything else group 0, and each segment is ordered by
    (level, launch rank, build index)."""
    from implicit_depth_amd import _lib, nhwc

    def op(kind, tile_m=0, tile_n=0):
        o = nhwc.Op()
        o.kind, o.N, o.Ho, o.Wo, o.Cout, o.tile_m, o.tile_n, o.split_k = kind, 1, 8, 16, 64, tile_m, tile_n, 1
        return o

    A, B_, D, E = 0xA000, 0xB000, 0xD000, 0xE000
    plan = [  # (op, reads, writes)
        (op(nhwc.OP_IMPORT), [], [(A, 0, 64)]),                                  # 0  segment 0
        (op(nhwc.OP_CONV, 8), [(A, 0, 64)], [(B_, 0, 64)]),                      # 1  8-row LDS conv: runs alone
        (op(nhwc.OP_CONV, 9, 2), [(A, 0, 64)], [(B_, 64, 128)]),                 # 2  4-row LDS conv, 32-channel tiles
        (op(nhwc.OP_CONV, nhwc.TILE_WINO), [(A, 0, 32)], [(D, 0, 64)]),          # 3  F(2x2): leads its level
        (op(nhwc.OP_CONV, 9, 0), [(A, 32, 64)], [(D, 64, 128)]),                 # 4  4-row LDS conv, 64-channel tiles: before op 2
        (op(nhwc.OP_EXPORT), [(B_, 0, 128)], []),                                # 5
        (op(nhwc.OP_CONV, nhwc.TILE_WINO4), [(B_, 0, 64)], [(E, 0, 64)]),        # 6  segment 1: reads what op 1 wrote, yet starts at level 0
        (op(nhwc.OP_UPSAMPLE2), [(D, 0, 64)], [(A, 0, 64)]),                     # 7  level 0 of its segment (ops 0-4 touching A are in the other one)
        (op(nhwc.OP_CONV, 1, 4), [(E, 0, 64)], [(D, 0, 64)]),                    # 8  after 6 (read after write) and 7 (write after read)
        (op(nhwc.OP_HEAD), [(D, 0, 16)], []),                                    # 9
    ]
    ops = (nhwc.Op * len(plan))(*[p[0] for p in plan])
    regions, offs = [], [0]
    for _, reads, writes in plan:
        for rs in (reads, writes):
            regions += [x for r in rs for x in r]
            offs.append(len(regions) // 3)
    n = len(plan)
    order, levels = (C.c_int32 * n)(), (C.c_int32 * n)()
    reg, off = (C.c_uint64 * len(regions))(*regions), (C.c_int32 * len(offs))(*offs)
    L = _lib.lib()
    assert L.idh_schedule_ops(ops, n, 6, reg, off, nhwc.SCHED_MERGE_LEVELS | nhwc.SCHED_WINO_GROUP, order, levels) == 0
    assert list(order) == [0, 3, 4, 2, 1, 5, 7, 6, 8, 9]
    assert list(levels) == [0, 1, 1, 1, 1, 2, 0, 0, 1, 2]
    assert [o.group for o in ops] == [1, 2, 2, 2, 0, 0, 1, 0, 2, 0]
    assert [(o.kind, o.tile_m) for o in ops] == [(plan[k][0].kind, plan[k][0].tile_m) for k in order], "the ops moved with the permutation"
    # without the two flags: the import, the upsampling and the direct conv run alone and the F(2x2) conv is ordered like any other op
    ops = (nhwc.Op * n)(*[p[0] for p in plan])
    assert L.idh_schedule_ops(ops, n, 6, reg, off, 0, order, None) == 0
    assert list(order) == [0, 4, 2, 1, 3, 5, 6, 7, 8, 9] and [o.group for o in ops] == [0, 2, 2, 0, 0, 0, 0, 0, 0, 0]
    # one segment: op 7 now waits for every earlier op that touches A's channels, op 6 for op 1
    ops = (nhwc.Op * n)(*[p[0] for p in plan])
    assert L.idh_schedule_ops(ops, n, 0, reg, off, 3, order, levels) == 0
    assert list(levels) == sorted(levels) and levels[list(order).index(6)] == 2 and levels[list(order).index(7)] == 2
    assert L.idh_schedule_ops(None, 0, 0, None, None, 3, None, None) == 0 and L.idh_schedule_ops(None, 2, 0, reg, off, 3, None, None) == -1


def test_plan_schedule_goes_through_the_library():
    """nhwc.Plan.schedule_segments keeps its bookkeeping: ``levels``, ``meta`` and the build-index map follow the library's permutation."""
    import torch

    from implicit_depth_amd import nhwc

    p = nhwc.Plan(torch.device("cpu"))
    a, b, c = p.buffer(1, 8, 16, 32), p.buffer(1, 16, 32, 32), p.buffer(1, 8, 16, 32)
    i_exp = p.export_nchw(b)
    p.upsample2(a, b)  # writes what the export reads: one level later
    i_imp = p.import_nchw((1, 32, 8, 16), c)
    assert p.schedule_segments(0) == 0
    assert [op.kind for op in p.ops] == [nhwc.OP_IMPORT, nhwc.OP_EXPORT, nhwc.OP_UPSAMPLE2] and p.levels == [0, 0, 1]
    assert (p._idx(i_exp), p._idx(i_imp)) == (1, 0) and [len(m["writes"]) for m in p.meta] == [1, 0, 1]
    assert [op.group for op in p.ops] == [1, 0, 2]
