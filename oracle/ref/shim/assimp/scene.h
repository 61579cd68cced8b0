/* Host stand-in for <assimp/scene.h>: forward declarations of the types the
 * reference's Scene class names in its member signatures. */
#ifndef PTREF_SHIM_ASSIMP_SCENE_H
#define PTREF_SHIM_ASSIMP_SCENE_H
struct aiScene;
struct aiNode;
struct aiMesh;
#endif
