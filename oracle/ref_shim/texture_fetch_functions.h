/* texture_fetch_functions.h -- empty stand-in: tex2D is declared in cuda_runtime.h. */
#pragma once
#include "cuda_runtime.h"
