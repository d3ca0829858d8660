// fir_internal.h — what the FIR translation units call in one another (C++ linkage, library-private).
#pragma once
#include <hip/hip_runtime.h>
#include "art_internal.h"

int  artfir_general (const ArtFirArgs &a, const ArtSegTable &segs, hipStream_t st);                 // fir_general.hip; -1: span does not fit the LDS
void artfir_strict (const ArtFirArgs &a, const ArtSegTable &segs, int precise, hipStream_t st);      // fir_general.hip
bool artfir_takes_matrix_path (const ArtFirArgs *a, const ArtSegTable *segs, int kernel_pref, bool sizing = false);   // fir_matrix.hip | fir_matrix64.hip
int  artfir_matrix (const ArtFirArgs *a, const ArtSegTable *segs, int kernel_pref, void *stream);    // fir_matrix.hip | fir_matrix64.hip
void artfir_matrix_needs (const ArtFirArgs *a, const ArtSegTable *first, int kernel_pref, ArtFirNeeds *n);   // fir_matrix.hip | fir_matrix64.hip (nothing)
void artfir_rows_touch (const ArtFirArgs *a, const ArtSegTable *segs);                               // fir_matrix.hip | fir_matrix64.hip (nothing)
bool artfir_test_fail ();                                                                             // fir_dispatch.hip: the ARTAMD_TEST_FAIL_FIR hook, one count per FIR launch
// many calls of one shape as one launch of the f32 streaming matrix kernel (fir_matrix.hip; the 8-byte build has no such kernel: never planned)
int    artfir_group_plan (const ArtFirArgs *a, const ArtSegTable *segs, int kernel_pref, ArtFirGroupCall *out);   // fir_matrix.hip | fir_matrix64.hip (0)
int    artfir_group_same_class (const ArtFirGroupCall *x, const ArtFirGroupCall *y);
size_t artfir_group_table_bytes (int n);
int    artfir_group (const ArtFirGroupCall *calls, int n, void *d_table, void *stream);
