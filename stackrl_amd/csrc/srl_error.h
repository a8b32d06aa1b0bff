// srl_error.h — how a launching export of libstackrl_qnet.so ends: `refused` (1) before anything is launched, or `launched`
// after its last launch: 0, or 2 with "<what>: <the HIP error>".  The text goes to the file's own thread_local buffer (each
// .hip file keeps its buffer and its `srl_*_last_error` accessor: they are ABI).
#ifndef SRL_ERROR_H_
#define SRL_ERROR_H_

#include <hip/hip_runtime.h>
#include <stdio.h>

// a call refused for its arguments: 1, with "<what>: bad arguments<takes>" (`takes`: what the export accepts, or "")
template <size_t N>
static inline int refused(char (&err)[N], const char* what, const char* takes) {
  snprintf(err, N, "%s: bad arguments%s", what, takes);
  return 1;
}

template <size_t N>
static inline int launched(char (&err)[N], const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(err, N, "%s: %s", what, hipGetErrorString(e)); return 2; }
  return 0;
}

#endif
