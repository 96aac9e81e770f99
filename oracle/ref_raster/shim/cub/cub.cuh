// cub -> hipcub: DeviceScan::InclusiveSum and DeviceRadixSort::SortPairs keep cub's signatures (rocPRIM's radix sort is a
// stable LSD sort, like cub's).
#pragma once
#include <hipcub/hipcub.hpp>
namespace cub = hipcub;
