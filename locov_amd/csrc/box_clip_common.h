// Boxes.clip's clamp, ONE copy: users image_batch.hip (locov_detector_rescale) and proposal_map.hip (locov_map_proposals).
#pragma once
#include "common.h"

namespace locov {

__device__ __forceinline__ float clamp_like_torch(float v, float hi)      // clamp(min=0, max=hi): NaN stays NaN
{
    return v != v ? v : fminf(fmaxf(v, 0.f), hi);
}

}  // namespace locov
