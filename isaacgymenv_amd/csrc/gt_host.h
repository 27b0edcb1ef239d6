// gt_host.h -- host helpers shared by libgymtask's sources (defined in gt_anymal.hip, next to gt_last_error).
#pragma once

// sets the calling thread's gt_last_error text
void gt_set_last_error(const char* msg);
// after a kernel launch: 0, or -1 with "<where>: <hipGetErrorString>" as the last error
int gt_launched(const char* where);
