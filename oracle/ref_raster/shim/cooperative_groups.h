// The reference uses this_grid().thread_rank(), this_thread_block() and block.sync() only: HIP's cooperative groups
// provide them under the same namespace.
#pragma once
#include <hip/hip_cooperative_groups.h>
