// ORACLE — TEST INFRASTRUCTURE ONLY.  AddressSanitizer / UndefinedBehaviourSanitizer run of orc_test_physics_interaction on the two poses
// in which the reference's intersectCapsule (bounding_volumes.cpp:363-384) hands intersectCylinder (:295-361) a distance that nobody
// has written: the origin radially inside the infinite cylinder and no cap disk taken.  Built and run by `make -C oracle sanitize-rays`;
// prints what each pose pushed, for any optimisation level, and exits 0 if that is what the cylinder collider gets in the same pose.
#include "oworld.cpp"
#include <cstdio>

using namespace orc;

static int cast(const char* name, const float* spherePos, const float* capsulePos, const float* origin, const float* direction)
{
	const float mat[3] = { 0.1f, 0.5f, 1.f }, ident[4] = { 0.f, 0.f, 0.f, 1.f };
	world* w = orc_world_create();
	// body 0: a sphere far down the ray (a clean hit at t = 19.5, the value a stale stack slot may well hold); body 1: the capsule
	const float sphere[10] = { 0.f, 0.f, 0.f, 0.5f };
	const float capsule[10] = { 0.f, -1.f, 0.f, 0.f, 1.f, 0.f, 0.25f };
	u32 b0 = orc_add_body(w, 0, 0.f, 0.f, 0.f, spherePos, ident);
	orc_add_collider(w, b0, 0, sphere, mat);
	u32 b1 = orc_add_body(w, 0, 0.f, 0.f, 0.f, capsulePos, ident);
	orc_add_collider(w, b1, 1, capsule, mat);
	u32 pushed = orc_test_physics_interaction(w, origin, direction, 1000.f);
	float acc[12];
	orc_read_accumulators(w, acc);
	printf("%s: pushed %d, force of it (%g %g %g), torque (%g %g %g)\n", name, (int)pushed - 1,
		pushed ? acc[6 * (pushed - 1)] : 0.f, pushed ? acc[6 * (pushed - 1) + 1] : 0.f, pushed ? acc[6 * (pushed - 1) + 2] : 0.f,
		pushed ? acc[6 * (pushed - 1) + 3] : 0.f, pushed ? acc[6 * (pushed - 1) + 4] : 0.f, pushed ? acc[6 * (pushed - 1) + 5] : 0.f);
	orc_world_destroy(w);
	return (int)pushed - 1;
}

int main()
{
	// A: origin inside the capsule's cylinder part, ray perpendicular to the axis (d.y == 0 exactly): the cylinder reports a hit at the
	//    unwritten distance; started at 0 the capsule (body 1) is the closest hit, as it is for a cylinder collider in the same pose.
	const float sphereA[3] = { 20.f, 0.f, 0.f }, posA[3] = { 0.f, 0.f, 0.f }, originA[3] = { 0.125f, 0.25f, 0.f }, dirA[3] = { 1.f, 0.f, 0.f };
	int a = cast("A inside, perpendicular", sphereA, posA, originA, dirA);
	// B: origin radially inside, 1.5 above the upper end, ray leaving sideways and slightly downwards: it misses the capsule by more than a
	//    metre, and the cap disk is not taken; y = o.y + t * d.y lands inside the cylinder's height for an unwritten t in about [15, 35].
	const float sphereB[3] = { 20.f, 0.75f, 0.f }, posB[3] = { 0.f, 0.25f, 0.f }, originB[3] = { 0.125f, 2.75f, 0.f }, dirB[3] = { 0.9950371902f, -0.0995037190f, 0.f };
	int b = cast("B beyond the end, sideways", sphereB, posB, originB, dirB);
	return (a == 1 && b == 0) ? 0 : 1;
}
