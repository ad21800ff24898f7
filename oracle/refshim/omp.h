// The reference loop is compiled WITHOUT OpenMP: it mutates a shared map inside its parallel loop, so serial execution
// is its defined behaviour.  TEST INFRASTRUCTURE ONLY.
#pragma once
static inline int omp_get_thread_num(void) { return 0; }
static inline int omp_get_max_threads(void) { return 1; }
