#pragma once
#include "cuda_to_hip.h"
