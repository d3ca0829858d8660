// staging.hip.h — pinned staging of the argument tables of the multi-item launches (FIR batch and schedule; arthip_table_upload for the rest).
// C++ linkage, library-private; defined in device_rt.hip.
#pragma once
#include <hip/hip_runtime.h>

// Per calling thread, kept: a table goes to the device without the runtime's bounce through its own pinned buffers.  Two tables
// take turns, each guarded by an event recorded after the copies out of it: the call returns without waiting for the stream, and
// the host plans the next one while this one runs.
struct Staging { void *host; size_t cap; hipEvent_t ev; bool pending; };

// the next turn's table, of `bytes` bytes at least (nullptr: out of memory)
Staging *staging_take (size_t bytes);
// the table must outlive the asynchronous copies out of it: marked here, waited for before its next turn.  -1: neither could be made sure of
int staging_give (Staging *sg, hipStream_t st);
