/* device_launch_parameters.h -- empty stand-in: blockIdx, blockDim and threadIdx are declared in cuda_runtime.h. */
#pragma once
#include "cuda_runtime.h"
