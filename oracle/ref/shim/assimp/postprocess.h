/* Host stand-in for <assimp/postprocess.h>: nothing the bridge compiles uses it. */
#ifndef PTREF_SHIM_ASSIMP_POSTPROCESS_H
#define PTREF_SHIM_ASSIMP_POSTPROCESS_H
#endif
