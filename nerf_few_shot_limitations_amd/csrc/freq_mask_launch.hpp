// freq_mask_launch.hpp -- the two masked launches of freq_mask.hip, called from train_shared.hip in place of the plain ones
#pragma once
#include "freq_mask.hpp"
#include "train_shared_core.hpp"

namespace nrf {

// repack3_kernel's launch (same argument block, same grid) with the masked elements scaled in front of the conversion
void launch_repack3_masked(const float* flat, const Repack3Args& a, unsigned grid, const FreqMaskArgs& f, hipStream_t s);
// weight_grad_reduce_kernel's launch with each masked weight's sum scaled in front of its add
void launch_weight_grad_reduce_masked(const GradKArgs& g, const FreqMaskArgs& f, hipStream_t s);

}  // namespace nrf
