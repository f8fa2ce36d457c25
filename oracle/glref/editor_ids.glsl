#version 430 core
// editor_ids.glsl -- NOT RayZen's shader: the ID pass of oracle/glref's editor mode.  It runs behind RayZen's own
// editor_vertex.glsl with the same draws and depth test as the colour pass, and writes what the colour pass's fragment shader
// was given: which object (uObjectIndex, set per draw by the harness), which triangle of its mesh (gl_PrimitiveID: the draw
// is glDrawArrays(GL_TRIANGLES) over the mesh's triangles in order), the flat material index, the interpolated world position
// and normal, and the window depth.  The input block is not written here: glref.c replaces the next line with the one that
// RayZen's editor_fragment.glsl declares, read at run time, so that the interface matches editor_vertex.glsl's output.
GLREF_FRAGMENT_INPUTS
uniform int uObjectIndex;
layout(location = 0) out ivec4 ids;
layout(location = 1) out vec4 posDepth;
layout(location = 2) out vec4 normalOut;
void main() {
    ids = ivec4(uObjectIndex, gl_PrimitiveID, fs_in.materialIndex, 1);
    posDepth = vec4(fs_in.worldPos, gl_FragCoord.z);
    normalOut = vec4(fs_in.normal, 0.0);
}
