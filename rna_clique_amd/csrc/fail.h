// The library's one error path (no HIP here: the .cpp files include it too).
#pragma once
#include <string>

// engine.hip: keeps msg for rc_last_error() and returns code
int rcg_fail(int code, const std::string &msg);
