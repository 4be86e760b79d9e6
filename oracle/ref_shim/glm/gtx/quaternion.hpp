/* glm/gtx/quaternion.hpp -- stand-in: quat, quat * quat, angleAxis and mat4_cast are defined in glm.hpp. */
#pragma once
#include "../glm.hpp"
