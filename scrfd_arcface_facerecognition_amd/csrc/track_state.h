// The tracker's host-side handle (track.hip), shared with the best-shot keeper (shots.hip), which reads the tracker's slots and the stream
// table of its last step.  Not part of the ABI.
#pragma once
#include "common.h"

struct fid_tracker {
    int S = 0, T = 0, device = 0;
    int32_t *slots = nullptr;                // [S][T][FID_TRACK_SLOT_WORDS]
    int32_t *streams = nullptr;              // [S][2] = {next_id, lost}
    int32_t *tab = nullptr;                  // [tab_cap] stream of frame b | [tab_cap] EMBED-flagged faces of frame b
    int tab_cap = 0;
    bool pending = false;                    // a step whose identify has not run
    int B = 0, cap = 0, row_cap = 0;         // ... and its shape
    std::vector<int32_t> stream;             // ... and its stream array
    unsigned long long serial = 0;           // steps so far: fid_track_keep takes each step at most once
};
