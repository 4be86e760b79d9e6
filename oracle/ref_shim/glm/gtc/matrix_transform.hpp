/* glm/gtc/matrix_transform.hpp -- stand-in: the reference's kernel headers include it and use nothing of it. */
#pragma once
#include "../glm.hpp"
